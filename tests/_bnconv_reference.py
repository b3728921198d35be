"""Float64 statement of the three ResNet-50 kernels that fold BatchNorm into a neighbouring 1x1 convolution, the inputs of their
tests, and the comparisons (tests/ only; torch alone, nothing of this library, CPU or GPU tensors alike).  Used by
tests/test_gpu_bnconv_reference.py (the kernels) and tests/test_bnconv_reference_host.py (an fp32 model of the kernels' arithmetic,
honest and with planted faults: the proof that the comparisons reject what they should and accept what they should).

The operations, from the kernel headers:

    bnload (csrc/conv_bnload.hip):   sc = rstd gamma, sh = beta - mean sc
                                     y = round16(relu(t sc + sh (+ res | + round16(res sc_r + sh_r))))       bits = (y > 0)
                                     out = round16(y W^T),  S0 / S1 = column sum / sum of squares of the ROUNDED out
                                     mean = S0 / M, rstd = 1 / sqrt(S1 / M - mean^2 + eps), running stats as nn.BatchNorm2d
    bnbwd  (csrc/conv_bnbwd.hip):    g = dy keep,  xhat = (t - mean) rstd,  ka = gamma rstd,  kb = fl32(dbeta fl32(1 / M)), kg likewise
                                     dt = round16(ka (g - kb - xhat kg)),  dx = round16(dt16 W),  gw = dt16^T x (fp32)
                                     bnred: sum and sum-times-xhat2 of dx16 under bits2,  xhat2 = (t2 - mean2) rstd2
    bnred GEMM (csrc/gemm_expand.hip): dx = round16(a W + addend under bits), the same two sums of dx16

Two kinds of input.

"exact": everything on the k / 4 grid of tests/_exact_grid.py, rstd and gamma signed powers of two (both signs), so that every
intermediate of the apply arithmetic is exactly representable in fp32 whether or not the compiler contracts to fma, and every stored
16-bit value is the float64 value rounded once.  The weights of the contractions are small INTEGERS (k / 4 times 4), sparse where a
long sum over the M rows follows (statistics, bnred, gw), so that the terms of those sums stay on the 1/16 grid: check_exact asserts
from the data that each sum of magnitudes stays below 2^20 (plain fp32 additions) or B_MFMA (through the matrix units).  The
backward coefficients: M a power of two and dbeta = M j / 4 give kb = j / 4 exactly; at ragged M a random half of the channels has
dgamma = dbeta = 0 (bit-checked), the other half keeps M j / 4 (kb, kg then carry fp32 roundings: per-element bar) and has zero
weight rows, so that dx and bnred stay exact.  So the ragged exact case does NOT cover every channel: the dt of that other half reaches
neither dx nor the bnred sums there, and in the weight-gradient form it is seen only through gw under the widened bar; the
Gaussian kind at the same M carries those channels through every output.  Outputs are then compared AS BITS (values: -0 == +0, a NaN never equals).

"gauss": the inputs of the older kernel-against-kernel files, rounded to storage first.  With u = 2^-24 and gamma_n = n u / (1 - n u):
* y:  |got - ref| <= ulp16(max(|got|, |ref|)) / 2 + gamma_5 (|t sc| + |mean sc| + |beta| + |r|) + tie.  The fp32 chain rounds sc,
  mean sc, beta - ., t sc, . + sh, . + r: at most 5 roundings lie on the path of any term (fewer when contracted).  `got` is the
  fp32 value rounded once, so it lies within half a 16-bit step (at |got|) of a value within the fp32 bar of the reference; the
  reference is NOT rounded, so no boundary term is needed for y itself.  tie: with the branch BatchNorm (RES = 2) the residual is
  itself rounded to 16 bits; its fp32 value lies within gamma_4 (|res sc_r| + |mean_r sc_r| + |beta_r|) + u |r| of the float64 one,
  so the kernel's 16-bit residual lies between round16 of the two ends of that interval: tie = their distance (0 almost everywhere).
* dt: the same with gamma_6 |ka| (|g| + |kb| + |xhat kg|): xhat has 2 roundings, xhat kg 3, g - kb 1, the difference 1, ka 1, the
  product 1: at most 6 on a path.  kb and kg are computed in fp32 by the reference exactly as the kernel does.
* keep bits: equal to y_got > 0 exactly; they differ from (float64 pre-activation > 0) only where |pre-activation| <= its fp32 bar.
* out, dx: the reference contracts the 16-bit y / dt THE KERNEL WROTE (each tied to float64 above):
  ulp16 / 2 + gamma_K sum |a b| (+ |addend| for the GEMM, gamma_(K + 1)).
* dx of the weight-gradient form: dt is never written.  The reference contracts round16(float64 dt); the kernel's 16-bit dt lies
  between round16(dt - E) and round16(dt + E) (E the fp32 bar above + u |dt|), and the bar is widened by sum_k |W| (that distance).
  This bar is loose wherever a dt sits near a rounding boundary (a whole 16-bit step of dt times |W|): the exact cases carry
  the weight-gradient form bit for bit.  gw likewise: gamma_n sum |dt16 x| + sum_m (that distance) |x|.
* sums over rows (statistics, bnred, gw): gamma_n sum |terms|, n from the kernel's structure (the callers count it): trips of a
  workgroup over its row tiles, the in-wavefront exchange (4 steps over 16 lanes), the wavefronts of the workgroup, the roundings
  inside a term, one final rounding; the folds over workgroups run in fp64 (bn_stats / bn_bwd finish) or along chains of groups / 16
  + 16 (wgrad1x1_fold).
* mean, rstd, running statistics: from the bars dS0, dS1 of the sums as tests/test_gpu_bn_reference.py derives them:
  |d mean| <= dS0 / M + u |mean|, |d var| <= (dS1 + 2 |mean| dS0) / M = r (var + eps), rstd within (1 - r)^(-1/2) - 1 + 2 u.

Rows past M of every input allocation hold a large finite poison with all keep bits set: a leaked row is not masked away.
"""
import types

import torch

from tests._exact_grid import B_MFMA, assert_same, check_exact, gen, grid, ulp16

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
POISON = 3.0e4                 # large, finite in fp16 and bf16
TAIL_ROWS = 64
EPS = 1e-5
EPS64 = float(torch.tensor(EPS, dtype=F32))
MOM = 0.1
MOM32 = float(torch.tensor(MOM, dtype=F32))
ONE_MINUS_MOM = float(torch.tensor(1.0, dtype=F32) - torch.tensor(MOM, dtype=F32))


def gamma_n(n):
    return n * U / (1 - n * U)


def round16(v, dtype):
    """float64 -> 16 bits as torch does it (through fp32, RNE both times)."""
    return v.float().to(dtype)


def pack_bits(keep):
    """bool [.., 8 j] -> bytes, bit i of a byte = element 8 b + i."""
    b = keep.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32, device=keep.device)
    return b.sum(1).to(torch.uint8)


def unpack_bits(bits, shape):
    b = (bits.to(torch.int32).unsqueeze(1) >> torch.arange(8, dtype=torch.int32, device=bits.device)) & 1
    return b.reshape(shape).bool()


def ulp32(v):
    _, e = torch.frexp(v.abs())
    return torch.pow(2.0, (e - 24).double())


class Worst(dict):
    """Worst |error| / bar per compared quantity."""

    def note(self, name, ratio):
        self[name] = max(self.get(name, 0.0), float(ratio))

    def merge(self, other):
        for k, v in other.items():
            self.note(k, v)

    def __str__(self):
        return ", ".join("%s %.3f" % kv for kv in sorted(self.items()))


def close(got, ref, bar, name, what, worst, half=None):
    """|got - ref| <= bar element by element (a NaN fails); notes the worst ratio.  half: the half-ulp16 term of a 16-bit output's
    bar (a rounding tie sits on it, so the ratio to the whole bar reaches 1 for correct code): the part of the error past it is
    also noted as a fraction of the REST of the bar, under `name + " fp32 term"`."""
    d = (got.double() - ref).abs()
    ok = d <= bar
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bar)
    if half is not None and bool(ok.all()):
        over = (d - half).clamp_min(0.0)
        worst.note(name + " fp32 term", torch.where(over == 0, torch.zeros_like(d), over / (bar - half)).max())
    if not bool(ok.all()):
        idx = torch.nonzero(~ok)[:4]
        first = tuple(idx[0].tolist())
        raise AssertionError("%s %s: %d of %d elements past the bar, first at %s (got %r, want %r, bar %g); more at %s" % (
            what, name, int((~ok).sum()), ok.numel(), first, float(got[first]), float(ref[first]), float(bar[first]), idx[1:].tolist()))
    worst.note(name, ratio.max())


def same(got, want, name, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s %s: %s %s against %s %s" % (
        what, name, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    assert_same(got, want, "%s %s" % (what, name))


def bar16(got, ref, dtype):
    return 0.5 * ulp16(torch.maximum(got.double().abs(), ref.abs()), dtype)


def on_grid(t, per_unit, what):
    v = t.double() * per_unit
    assert torch.equal(v, torch.round(v)), "%s off the 1/%d grid" % (what, per_unit)


def contraction_exact(a_abs_b_abs, what):
    """The sum of magnitudes of every output of a contraction through the matrix units is below B_MFMA."""
    worst = float(a_abs_b_abs.max())
    assert worst < B_MFMA, "%s: sum of magnitudes %g: the fp32 sums would not be exact" % (what, worst)


# ---------------------------------------------------------------- inputs
def rows(vals, tail=TAIL_ROWS):
    """[m, c] as the head of an allocation of m + tail rows whose tail holds POISON."""
    m, c = vals.shape
    big = torch.full((m + tail, c), POISON, dtype=vals.dtype, device=vals.device)
    big[:m] = vals
    return big[:m]


def keep_rows(keep, tail=TAIL_ROWS):
    """Packed keep bits of [m, c] as the head of an allocation whose tail rows keep everything."""
    m, c = keep.shape
    big = torch.ones((m + tail, c), dtype=torch.bool, device=keep.device)
    big[:m] = keep
    return pack_bits(big)[:m * c // 8]


def past_end(view, nrows=1):
    """The first rows behind a view made by rows() (the poison), for the host model's planted faults."""
    m, c = view.shape
    return torch.as_strided(view, (m + nrows, c), (c, 1))[m:]


def pow2(n, seed, dev, exps=(0, 1)):
    """Signed powers of two, both signs present."""
    g = gen(dev, seed)
    e = torch.tensor(exps, dtype=F32, device=dev)[torch.randint(0, len(exps), (n,), generator=g, device=dev)]
    sign = torch.randint(0, 2, (n,), generator=g, device=dev).float() * 2 - 1
    sign[0], sign[1] = 1.0, -1.0
    return sign * torch.pow(2.0, e)


def ints(shape, seed, dtype, dev, kmax, density=1.0):
    """Small integers |k| <= kmax (the k / 4 grid times 4), sparse with density < 1."""
    return (grid(shape, seed, F32, dev, kmax=kmax, density=density) * 4).to(dtype)


def _randn(shape, g, dev, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g, device=dev) * scale + shift


def _gauss_bn(c, g, dev):
    return (_randn((c,), g, dev, 0.1), torch.rand(c, generator=g, device=dev) + 0.5, torch.rand(c, generator=g, device=dev) + 0.5,
            _randn((c,), g, dev, 0.1))


def _exact_bn(c, seed, dev):
    """mean on k / 4 (|k| <= 1), rstd in +-{1, 2}, gamma = +-1, beta on k / 4 (|k| <= 2): y stays on the 1/4 grid, small enough
    for the sums of out^2 over 65,000 rows."""
    return (grid((c,), seed, F32, dev, kmax=1), pow2(c, seed + 1, dev), pow2(c, seed + 2, dev, exps=(0,)),
            grid((c,), seed + 3, F32, dev, kmax=2))


def bnload_inputs(kind, dtype, dev, m, k, n, resmode, seed):
    """resmode 0: no residual, 1: residual tensor, 2: residual through its own BatchNorm.  w [N, K] (k contiguous)."""
    s = types.SimpleNamespace(kind=kind, dtype=dtype, m=m, k=k, n=n, resmode=resmode, res=None, bnr=None, w_dense=None)
    if kind == "exact":
        s.t = rows(grid((m, k), seed, dtype, dev, kmax=2))
        if resmode:
            s.res = rows(grid((m, k), seed + 1, dtype, dev, kmax=2))
        s.w = ints((n, k), seed + 2, dtype, dev, 1, density=3.0 / k)          # sparse +-1: out on the 1/4 grid, out^2 on 1/16
        s.w_dense = grid((n, k), seed + 3, dtype, dev, kmax=4)                # dense k / 4: the contraction alone
        s.bn = _exact_bn(k, seed + 4, dev)
        if resmode == 2:
            s.bnr = _exact_bn(k, seed + 8, dev)
    else:
        g = gen(dev, seed)
        s.t = rows(_randn((m, k), g, dev).to(dtype))
        if resmode:
            s.res = rows(_randn((m, k), g, dev).to(dtype))
        s.w = _randn((n, k), g, dev, 0.1).to(dtype)
        s.bn = _gauss_bn(k, g, dev)
        if resmode == 2:
            s.bnr = _gauss_bn(k, g, dev)
    g = gen(dev, seed + 12)
    s.rm0, s.rv0 = torch.randn(n, generator=g, device=dev), torch.rand(n, generator=g, device=dev) + 0.5
    return s


BK, BN = 256, 64               # the one shape of csrc/conv_bnbwd.hip


def bnbwd_inputs(kind, dtype, dev, m, masked, bred, seed):
    """K = 256, N = 64.  w [K, N] (n contiguous), x [M, N] the unit's saved input (behind a ReLU), bnred operands when bred."""
    s = types.SimpleNamespace(kind=kind, dtype=dtype, m=m, masked=masked, bred=bred, keep=None, bits=None, t2=None, keep2=None,
                              bits2=None, mean2=None, rstd2=None)
    g = gen(dev, seed)
    if masked:
        s.keep = torch.rand((m, BK), generator=g, device=dev) < 0.6
        s.bits = keep_rows(s.keep)
    if bred:
        s.keep2 = torch.rand((m, BN), generator=g, device=dev) < 0.5
        s.bits2 = keep_rows(s.keep2)
    if kind == "exact":
        s.t = rows(grid((m, BK), seed + 1, dtype, dev))
        s.dy = rows(grid((m, BK), seed + 2, dtype, dev))
        s.mean = grid((BK,), seed + 3, F32, dev)
        s.rstd, s.gamma = pow2(BK, seed + 4, dev), pow2(BK, seed + 5, dev)
        jb, jg = grid((BK,), seed + 6, F32, dev), grid((BK,), seed + 7, F32, dev)
        s.dbeta, s.dgamma = jb * m, jg * m                                    # M j / 4: exact in fp32 (M < 2^17)
        s.exact_ch = torch.ones(BK, dtype=torch.bool, device=dev)
        if m & (m - 1):
            s.exact_ch = torch.rand(BK, generator=g, device=dev) < 0.5
            s.dbeta, s.dgamma = s.dbeta * ~s.exact_ch, s.dgamma * ~s.exact_ch
        # dense integers for the contraction over K alone; sparse +-1 where the long bnred sums follow
        s.w = ints((BK, BN), seed + 8, dtype, dev, 1, density=3.0 / BK) if bred else ints((BK, BN), seed + 8, dtype, dev, 2)
        s.w = s.w * s.exact_ch.to(dtype).unsqueeze(1)
        s.x = rows(ints((m, BN), seed + 9, dtype, dev, 2, density=0.25).abs())
        if bred:
            s.t2 = rows(ints((m, BN), seed + 10, dtype, dev, 1))
            s.mean2 = ints((BN,), seed + 11, F32, dev, 1)
            s.rstd2 = pow2(BN, seed + 12, dev)
    else:
        s.t = rows(_randn((m, BK), g, dev).to(dtype))
        s.dy = rows(_randn((m, BK), g, dev, 0.01).to(dtype))
        s.x = rows(_randn((m, BN), g, dev, 1.0, 0.3).to(dtype).clamp_(min=0))
        s.w = _randn((BK, BN), g, dev, 1.0 / 16).to(dtype)
        s.gamma = torch.rand(BK, generator=g, device=dev) + 0.5
        td = s.t.double()
        s.mean = td.mean(0).float()
        s.rstd = (1.0 / torch.sqrt(td.var(0, unbiased=False) + EPS64)).float()
        gd = s.dy.double() * (s.keep if masked else 1.0)
        xh = (td - s.mean.double()) * s.rstd.double()
        s.dbeta, s.dgamma = gd.sum(0).float(), (gd * xh).sum(0).float()       # inputs of the fused kernel: the true sums
        s.exact_ch = torch.zeros(BK, dtype=torch.bool, device=dev)
        if bred:
            s.t2 = rows(_randn((m, BN), g, dev, 1.0, 0.2).to(dtype))
            t2d = s.t2.double()
            s.mean2 = t2d.mean(0).float()
            s.rstd2 = (1.0 / torch.sqrt(t2d.var(0, unbiased=False) + EPS64)).float()
    return s


def bnred_inputs(kind, dtype, dev, m, k, n, seed):
    """a [M, K], w [K, N] (n contiguous), addend [M, N] under keep1; the reduction of dx under keep2 against t2."""
    s = types.SimpleNamespace(kind=kind, dtype=dtype, m=m, k=k, n=n)
    g = gen(dev, seed)
    s.keep1 = torch.rand((m, n), generator=g, device=dev) < 0.5
    s.keep2 = torch.rand((m, n), generator=g, device=dev) < 0.6
    s.bits1, s.bits2 = keep_rows(s.keep1), keep_rows(s.keep2)
    if kind == "exact":
        s.a = rows(grid((m, k), seed + 1, dtype, dev, density=0.5))
        s.w = ints((k, n), seed + 2, dtype, dev, 2, density=3.0 / k)
        s.addend = rows(grid((m, n), seed + 3, dtype, dev))
        s.t2 = rows(grid((m, n), seed + 4, dtype, dev))
        s.mean2 = grid((n,), seed + 5, F32, dev)
        s.rstd2 = pow2(n, seed + 6, dev)
    else:
        s.a = rows(_randn((m, k), g, dev, 0.05).to(dtype))
        s.w = _randn((k, n), g, dev, k ** -0.5).to(dtype)
        s.addend = rows(_randn((m, n), g, dev, 0.05).to(dtype))
        s.t2 = rows(_randn((m, n), g, dev, 1.5, 0.3).to(dtype))
        t2d = s.t2.double()
        s.mean2 = t2d.mean(0).float()
        s.rstd2 = (1.0 / torch.sqrt(t2d.var(0, unbiased=False) + EPS64)).float()
    return s


# ---------------------------------------------------------------- comparisons
def _between(ref, e, dtype):
    """Distance between round16 of the two ends of [ref - e, ref + e]: how far two roundings of values in it can lie apart."""
    return (round16(ref + e, dtype).double() - round16(ref - e, dtype).double()).abs()


def bnload_apply_ref(s):
    """-> (float64 pre-activation, its fp32 bar)."""
    mean, rstd, gam, beta = [v.double() for v in s.bn]
    sc = rstd * gam
    t = s.t.double()
    pre = t * sc + (beta - mean * sc)
    mag = (t * sc).abs() + (mean * sc).abs() + beta.abs()
    tie = 0.0
    if s.resmode == 1:
        r = s.res.double()
    elif s.resmode == 2:
        mr, rr, gr, br = [v.double() for v in s.bnr]
        scr = rr * gr
        res = s.res.double()
        r64 = res * scr + (br - mr * scr)
        er = gamma_n(4) * ((res * scr).abs() + (mr * scr).abs() + br.abs()) + U * r64.abs()
        r = round16(r64, s.dtype).double()
        tie = _between(r64, er, s.dtype)
    if s.resmode:
        pre = pre + r
        mag = mag + r.abs()
    return pre, gamma_n(5) * mag + tie


def check_stats(s, got, out, n_chain, what, worst):
    """got.S [2, N] (float64: the partial rows summed), got.mean / rstd / rm / rv against the statistics of the rounded out."""
    m = s.m
    og = out.double()
    s0, s1 = og.sum(0), (og * og).sum(0)
    rmean = s0 / m
    var = (s1 / m - rmean * rmean).clamp_min(0.0)
    rrstd = 1.0 / torch.sqrt(var + EPS64)
    unb = var * m / (m - 1)
    ref_m = ONE_MINUS_MOM * s.rm0.double() + MOM32 * rmean
    ref_v = ONE_MINUS_MOM * s.rv0.double() + MOM32 * unb
    if s.kind == "exact":
        check_exact(og, og * og)
        same(got.S.float(), torch.stack([s0, s1]).float(), "S0 / S1", what)
        same(got.mean, rmean.float(), "mean", what)
        close(got.rstd, rrstd, ulp32(rrstd), "rstd (1 ulp)", what, worst)
        unb = unb.float().double()
        ref_m = ONE_MINUS_MOM * s.rm0.double() + MOM32 * got.mean.double()
        ref_v = ONE_MINUS_MOM * s.rv0.double() + MOM32 * unb
        close(got.rm, ref_m, 4 * U * (ONE_MINUS_MOM * s.rm0.double().abs() + MOM32 * got.mean.double().abs()), "running_mean (4u)", what, worst)
        close(got.rv, ref_v, 4 * U * (ONE_MINUS_MOM * s.rv0.double().abs() + MOM32 * unb.abs()), "running_var (4u)", what, worst)
        return
    d0, d1 = gamma_n(n_chain) * og.abs().sum(0), gamma_n(n_chain + 1) * s1
    close(got.S[0], s0, d0, "S0", what, worst)
    close(got.S[1], s1, d1, "S1", what, worst)
    close(got.mean, rmean, d0 / m + U * rmean.abs(), "mean", what, worst)
    dvar = (d1 + 2 * rmean.abs() * d0) / m
    r = dvar / (var + EPS64)
    assert float(r.max()) < 0.5, "%s: the variance bar is not small against the variance" % what
    close(got.rstd, rrstd, ((1 - r) ** -0.5 - 1 + 2 * U) * rrstd, "rstd", what, worst)
    close(got.rm, ref_m, 4 * U * (s.rm0.double().abs() + rmean.abs()) + MOM32 * d0 / m, "running_mean", what, worst)
    close(got.rv, ref_v, 4 * U * (s.rv0.double().abs() + unb.abs()) + MOM32 * dvar * m / (m - 1), "running_var", what, worst)


def bnload_check(s, got, n_chain, what, worst, dense=False):
    """got: y [M, K], bits [M K / 8], out [M, N] and, unless dense, S / mean / rstd / rm / rv.  dense: the run with s.w_dense
    (the contraction alone, exact kind only)."""
    pre, e = bnload_apply_ref(s)
    yref = pre.clamp_min(0.0)
    keep = unpack_bits(got.bits, pre.shape)
    assert bool((pre < 0).any()) and bool((pre > 0).any()), "%s: the ReLU clips nothing" % what
    odd = keep != (got.y > 0)
    assert not bool(odd.any()), "%s: keep bits != y > 0 at %s (y %s, float64 pre-activation %s)" % (
        what, torch.nonzero(odd)[:4].tolist(), got.y[odd][:4].tolist(), pre[odd][:4].tolist())
    if s.kind == "exact":
        same(got.y, round16(yref, s.dtype), "y", what)
        same(got.bits, pack_bits(pre > 0), "keep bits", what)
    else:
        h = bar16(got.y, yref, s.dtype)
        close(got.y, yref, h + e, "y", what, worst, half=h)
        off = keep != (pre > 0)
        assert bool((pre.abs()[off] <= e[off]).all()), "%s: keep bits differ from the float64 sign where it is certain" % what
    w = (s.w_dense if dense else s.w).double()
    yg = got.y.double()
    oref, omag = yg @ w.t(), yg.abs() @ w.abs().t()
    if s.kind == "exact":
        on_grid(yg, 4, "y")
        on_grid(w, 4, "w")
        contraction_exact(omag, what)
        same(got.out, round16(oref, s.dtype), "out (dense w)" if dense else "out", what)
    else:
        h = bar16(got.out, oref, s.dtype)
        close(got.out, oref, h + gamma_n(s.k) * omag, "out", what, worst, half=h)
    if not dense:
        check_stats(s, got, got.out, n_chain, what, worst)


def bnbwd_dt_ref(s):
    """-> (float64 dt, its fp32 bar)."""
    g = s.dy.double()
    if s.masked:
        assert not bool(s.keep.all()) and bool(s.keep.any()), "the mask masks nothing"
        g = g * s.keep
    inv_m = torch.tensor(1.0, dtype=F32, device=g.device) / torch.tensor(float(s.m), dtype=F32, device=g.device)
    kb, kg = (s.dbeta * inv_m).double(), (s.dgamma * inv_m).double()          # fp32 products, as the kernel forms them
    xhat = (s.t.double() - s.mean.double()) * s.rstd.double()
    ka = s.gamma.double() * s.rstd.double()
    ref = ka * (g - kb - xhat * kg)
    return ref, gamma_n(6) * ka.abs() * (g.abs() + kb.abs() + (xhat * kg).abs())


def check_dt(s, dt, what, worst, name="dt"):
    """A written dt [M, K] (the fused kernel's plain form, or the stand-alone bn_bwd): bits on the exact channels, the
    per-element bar on the others."""
    ref, e = bnbwd_dt_ref(s)
    ex = s.exact_ch
    if bool(ex.any()):
        same(dt[:, ex], round16(ref[:, ex], s.dtype), name, what)
    if not bool(ex.all()):
        nx = ~ex
        h = bar16(dt[:, nx], ref[:, nx], s.dtype)
        close(dt[:, nx], ref[:, nx], h + e[:, nx], name, what, worst, half=h)


def bnbwd_check(s, got, chains, what, worst):
    """got: dx [M, N]; dt [M, K] (plain form) or gw [K, N] fp32 (weight-gradient form); dg2 / db2 [N] when s.bred.
    chains: {"bnred": n, "gw": n}."""
    ref, e = bnbwd_dt_ref(s)
    ex = s.exact_ch
    exact = s.kind == "exact"
    w = s.w.double()
    wg = getattr(got, "dt", None) is None
    if wg:
        dt16 = round16(ref, s.dtype).double()
        tie = _between(ref, e + U * ref.abs(), s.dtype)
    else:
        check_dt(s, got.dt, what, worst)
        dt16 = got.dt.double()
        tie = torch.zeros_like(dt16)
    dxref, dxmag = dt16 @ w, dt16.abs() @ w.abs()
    if exact:
        on_grid(dt16[:, ex], 16, "dt16")
        on_grid(w, 1, "w")
        assert not bool(w[~ex].any()), "weight rows of the inexact channels must be zero"
        contraction_exact(dxmag, what)
        same(got.dx, round16(dxref, s.dtype), "dx", what)
    else:
        h = bar16(got.dx, dxref, s.dtype)
        close(got.dx, dxref, h + gamma_n(BK) * dxmag + tie @ w.abs(), "dx (wgrad form)" if wg else "dx", what, worst, half=h)
    if wg:
        x = s.x.double()
        gref, gmag = dt16.t() @ x, dt16.abs().t() @ x.abs()
        gbar = gamma_n(chains["gw"]) * gmag + tie.t() @ x.abs()
        if exact:
            on_grid(x, 1, "x")
            contraction_exact(gmag[ex], what)
            same(got.gw[ex], gref[ex].float(), "gw", what)
            if not bool(ex.all()):
                close(got.gw[~ex], gref[~ex], gbar[~ex], "gw", what, worst)
        else:
            close(got.gw, gref, gbar, "gw", what, worst)
    if s.bred:
        assert not bool(s.keep2.all()) and bool(s.keep2.any())
        check_bnred_sums(s, got, got.dx, BN, chains["bnred"], what, worst)


def check_bnred_sums(s, got, dx, n, n_chain, what, worst):
    """got.db2 / got.dg2 (fp32 [N]) against the sums of the stored dx under keep2."""
    g2 = dx.double() * s.keep2
    t2 = g2 * ((s.t2.double() - s.mean2.double()) * s.rstd2.double())
    sb, sg = g2.sum(0), t2.sum(0)
    if s.kind == "exact":
        check_exact(g2, t2)
        same(got.db2, sb.float(), "dbeta2", what)
        same(got.dg2, sg.float(), "dgamma2", what)
    else:
        close(got.db2, sb, gamma_n(n_chain) * g2.abs().sum(0), "dbeta2", what, worst)
        close(got.dg2, sg, gamma_n(n_chain + 3) * t2.abs().sum(0), "dgamma2", what, worst)


def bnred_check(s, got, n_chain, what, worst):
    """got: dx [M, N], dg2 / db2 [N]."""
    a, w = s.a.double(), s.w.double()
    add = torch.where(s.keep1, s.addend.double(), torch.zeros((), dtype=F64, device=a.device))
    assert not bool(s.keep1.all()) and bool(s.keep1.any()) and not bool(s.keep2.all()) and bool(s.keep2.any())
    ref, mag = a @ w + add, a.abs() @ w.abs() + add.abs()
    if s.kind == "exact":
        on_grid(a, 4, "a")
        on_grid(w, 1, "w")
        on_grid(add, 4, "addend")
        contraction_exact(mag, what)
        same(got.dx, round16(ref, s.dtype), "dx", what)
    else:
        h = bar16(got.dx, ref, s.dtype)
        close(got.dx, ref, h + gamma_n(s.k + 1) * mag, "dx", what, worst, half=h)
    check_bnred_sums(s, got, got.dx, s.n, n_chain, what, worst)
