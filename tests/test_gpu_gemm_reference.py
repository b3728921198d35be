"""The linear-layer GEMMs (csrc/gemm.hip, gemm_dma.hip, gemm8*.hip / gemm8_kernel.h, gemm_smallm.hip, gemm_expand.hip) against a
float64 restatement of the product and its epilogue, at the sizes the BERT-Large (T = 256 x 128 tokens) and DLRM (65,536 rows)
steps launch, over the WHOLE output.  GPU only.

Reference.  torch float64 on the GPU: a.double() @ b.double().T (or b.double(), or a.double().T @), the epilogue restated in
float64; nothing of this library.  Contractions of 32,768 terms and more are summed as a batch of row chunks (_tn).

Exactly summable inputs (tests/_exact_grid.py).  Operands, addends, mask sources and prior dw0 are k / 4 with small integer k,
biases fp32 multiples of 1/16, alpha a power of two: every term is a multiple of 1/16 (1/64 after the ACT_MUL source factor, 1/256
after the ACT_TANH_BWD one).  The float64 reference of |a| and |b| (+ |bias|, |addend|, |dw0|) is asserted below B_MFMA = 2^18
before any comparison, so every partial sum, in any order and any grouping (MFMA chains, K slices, slab folds, atomics), is exact
in fp32.  With |k| <= 4 the bound is at most K <= 65,536 by construction.  Then
* fp32 outputs (weight gradients, split-K, accumulate=True on a prior dw0) equal the float64 reference BIT FOR BIT;
* 16-bit outputs equal ref64.float().to(dtype) BIT FOR BIT (one RNE rounding of an exact fp32 value);
* that covers ACT_NONE, bias, ACT_RELU, ACT_RELU_BWD, ACT_ADD, ACT_ADD_MASKED, ACT_MUL, the pre-activation side output of ACT_GELU,
  the keep bits of gemm_relu_bits (= ref64 > 0) and ACT_TANH_BWD: gemm_dma.hip and gemm8_kernel.h evaluate it as g * (1 - y * y),
  and with y = k / 4, |y| <= 1, y * y and 1 - y * y are multiples of 1/16 in [0, 1], the product a multiple of 1/256 below 2^4:
  every intermediate is exact in fp32 (fused or not);
* gemm_colsum / gemm_colsum_bits: the column sums are fp32 additions of the STORED 16-bit dX (multiples of 1/16, or 1/64 for
  ACT_MUL); operands thinned (kmax = 2, density = 0.5) so that the column sums of |dX_ref| times the grid scale stay below 2^24,
  asserted from the reference alone: the sums are bit-exact too, accumulate=True included.

Transcendental epilogues (ACT_TANH, ACT_GELU, ACT_GELU_DAUX, ACT_GELU_BWD).  The pre-activation x is exact; the error is that of
the fp32 evaluation.  Bar: |got - f(x)| <= ulp16(max(|got|, |f|)) / 2 + E(x), E derived from the instruction list, u = 2^-24, each
fp32 add / multiply / fma one rounding (relative u), a rounded constant relative u, v_exp_f32 and v_rcp_f32 1 ulp = relative 2 u
(the accuracy the CDNA ISA guide documents for both).  First-order terms, times (1 + 2^-10) for the second-order ones (every
relative error below is under 200 u for |x| <= 45, beyond which exp2 saturates and the result is exactly +-1).
  fast_tanh(z) = 1 - 2 rcp(exp2(z c) + 1), c = fl(2 log2 e), T = tanh z  (common.h):
    a = fl(z c): relative 2 u; e = exp2(a): relative (2 ln2 |a| + 2) u = (4 |z| + 2) u; s = fl(e + 1): u; r = rcp(s): 2 u;
    the error of e reaches r scaled by e / (e + 1) = (1 + T) / 2, and 2 r = 1 - T; t = fl(1 - 2 r): u |T|:
    E_tanh(z) = u [ (1 - T^2) (2 |z| + 1) + 3 (1 - T) + |T| ].
  gelu(x) = x hp, hp = 0.5 (1 + th), th = fast_tanh(z), z = k0 (x + k1 x^3)  (gelu_tanh2 / gelu_tanh2_d, g8_gelu*):
    p = k1 x^3: 4 u (k1, three products); z: dz = u (4 k0 |p| + 3 |z|) (the sum, k0, the product);
    dT = (1 - T^2) dz + E_tanh(z);  E_gelu = 0.5 |x| dT + 2 u |gelu|  (1 + th and x hp round once each).
  gelu'(x) = hp + P, P = 0.5 x (1 - th^2) k0 q, q = 1 + 3 k1 x^2:
    S = 1 - th^2: dS = 2 |T| dT + u (T^2 + S);  dq = u (12 k1 x^2 + q);  dP = |0.5 x k0 q| dS + |0.5 x S k0| dq + 4 u |P|;
    E_gelu' = 0.5 dT + 0.5 (1 + T) u + dP + u |gelu'|.
  ACT_GELU_BWD = fl(g gelu'(y)): |g| E_gelu' + u |g gelu'|.
Each such test prints the worst observed excess over ulp16 / 2 beside the E at that element.  The inputs of these cases are thinned
(kmax = 1, density = 0.25) so that x spreads over about +-3 in steps of 1/16, where the functions bend.  What the bar can tell
apart: E is some 1e-6 |x| while ulp16 / 2 is 2^-9 (bf16) or 2^-12 (fp16) of the value, so a wrong constant shows only when it
moves the result by more than about half a 16-bit ulp (over |x| <= 3, k1 = 0.044 instead of 0.044715 passes the bar 74 times in
fp16 and 14 times in bf16; k1 = 0.0447 1.5 times in fp16 and not at all in bf16).

Which kernel ran.  Every case names the kernel its launch belongs to.  The test calls that kernel's `_try` entry point through the C
ABI, asserts return code 1 (and, for the ping-pong kernel, that dle_gemm8_launch_count() moved by one; for the tile kernels of
gemm_dma.hip, that it did not), then asserts that the public wrapper gives the same bits and counts the same way.  Each BERT / DLRM
case runs again with the ping-pong kernel pinned off (dle_gemm8_mode(0), restored in `finally`; the count must not move): the tile
kernels must be exact at the same sizes.  "legacy" is the register-staged gemm_kernel of gemm.hip: dle_gemm_dma_try must decline.

No stray writes.  Outputs, side outputs, keep bits and column sums are views at the head of over-long buffers filled with NaN
(0xFF bytes for the bits); the tail must keep its bits, a NaN left inside fails the comparison.

Realistic inputs (test_gaussian): x ~ N(0, 1), w ~ N(0, 1 / K) rounded to the 16-bit type, reference on the rounded values, the
Higham bars of tests/test_gpu_conv_reference.py with u = 2^-24, gamma_n = n u / (1 - n u):
* 16-bit outputs: ulp16 / 2 + gamma_(K + 2) sum |a b|.  The ping-pong kernel, the tile kernels and gemm_smallm.hip all keep ONE
  accumulator per output element and walk the K range in order (8- or 4-wave workgroups split the OUTPUT tile, not K; the
  ping-pong halves alternate K tiles into the same accumulators; gemm_smallm.hip streams the whole K range through one 16 x 16
  block per wavefront): chains of at most K additions, + alpha and bias;
* fp32 split-K outputs: gamma_n sum |a b|, n = ceil(K tiles / splitk) x 64 + splitk + 16 (gemm8_walk.h gives slice ky the K tiles
  [ky kt / s, (ky + 1) kt / s): at most ceil(kt / s); the slab fold adds at most ceil(s / 16) slabs in a chain, then 16 partials).
"""
import contextlib
import ctypes
import functools
import math
import zlib

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests._exact_grid import B_MFMA, Out, assert_same, bits as _bits, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DT_IDS = {BF: "bf16", HF: "fp16"}
U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32

# BERT-Large at the benchmarked batch: T tokens, hidden H, intermediate I, vocabulary V, B sequences, NM masked rows
T, H, I, V, B, NM = 32768, 1024, 4096, 30528, 256, 5120
MD = 65536                     # DLRM rows


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


# ---------------------------------------------------------------- float64 reference
def _tn(a, b, chunk=8192):
    """a [K, M]^T b [K, N] in float64, as a batch of row chunks."""
    a, b = a.to(F64), b.to(F64)
    if a.shape[0] < 32768:
        return a.t() @ b
    extra = -a.shape[0] % chunk
    if extra:
        a = torch.nn.functional.pad(a, (0, 0, 0, extra))
        b = torch.nn.functional.pad(b, (0, 0, 0, extra))
    k = a.shape[0] // chunk
    return torch.bmm(a.reshape(k, chunk, -1).transpose(1, 2), b.reshape(k, chunk, -1)).sum(0)


def _prod64(layout, a, b):
    """nt: a [m, k] b [n, k]; nn: a [m, k] b [k, n]; tn: a [k, m] b [k, n]."""
    if layout == "nt":
        return a.to(F64) @ b.to(F64).t()
    if layout == "nn":
        return a.to(F64) @ b.to(F64)
    return _tn(a, b)


def _shapes(layout, m, n, k):
    return {"nt": ((m, k), (n, k)), "nn": ((m, k), (k, n)), "tn": ((k, m), (k, n))}[layout]


def _pack_bits(keep):
    """bit (i n + j) & 7 of byte (i n + j) >> 3 = keep[i, j]."""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=keep.device)
    return (keep.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
SECOND_ORDER = 1.0 + 2.0 ** -10


def _tanh_err(z, t):
    return U * ((1 - t * t) * (2 * z.abs() + 1) + 3 * (1 - t) + t.abs())


def _gelu64(x):
    """(gelu, E_gelu, gelu', E_gelu') of float64 x: module docstring."""
    p = K1 * x ** 3
    z = K0 * (x + p)
    t = torch.tanh(z)
    y = 0.5 * x * (1 + t)
    dz = U * (4 * K0 * p.abs() + 3 * z.abs())
    dt = (1 - t * t) * dz + _tanh_err(z, t)
    ey = 0.5 * x.abs() * dt + 2 * U * y.abs()
    s, q = 1 - t * t, 1 + 3 * K1 * x * x
    ds = 2 * t.abs() * dt + U * (t * t + s)
    dq = U * (12 * K1 * x * x + q)
    pp = 0.5 * x * s * K0 * q
    dp = (0.5 * x * K0 * q).abs() * ds + (0.5 * x * s * K0).abs() * dq + 4 * U * pp.abs()
    d = 0.5 * (1 + t) + pp
    ed = 0.5 * dt + 0.5 * (1 + t) * U + dp + U * d.abs()
    return y, ey * SECOND_ORDER, d, ed * SECOND_ORDER


def _assert_within(got, ref, e, what):
    """|got - ref| <= ulp16(max(|got|, |ref|)) / 2 + e; prints the worst excess over ulp16 / 2 beside e there."""
    g = got.to(F64)
    assert bool(torch.isfinite(g).all()), "%s: non-finite output" % what
    half = 0.5 * ulp16(torch.maximum(g.abs(), ref.abs()), got.dtype)
    d = (g - ref).abs()
    excess = d - half
    i = int(torch.argmax(excess))
    print("%s: worst excess over ulp16/2 = %.3e with E = %.3e there (%d elements past ulp16/2, largest E %.3e)" % (
        what, float(excess.reshape(-1)[i]), float(e.reshape(-1)[i]), int((excess > 0).sum()), float(e.max())))
    bad = d > half + e
    assert not bool(bad.any()), "%s: %d elements past the bar, first %s: got %r want %r E %g" % (
        what, int(bad.sum()), torch.nonzero(bad)[0].tolist(), float(g[bad][0]), float(ref[bad][0]), float(e[bad][0]))


# ---------------------------------------------------------------- C ABI entry points that may decline
_VP, _I, _LL, _FL = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float


@functools.lru_cache(maxsize=None)
def _proto(name, res, *args):
    """A private prototype of one library symbol (the shared handle's argtypes are left alone)."""
    return ctypes.CFUNCTYPE(res, *args)((name, C.lib()))


def _count():
    return int(C.lib().dle_gemm8_launch_count())


@contextlib.contextmanager
def _pinned_off():
    setter = _proto("dle_gemm8_mode", _I, _I)
    old = setter(0)
    try:
        yield
    finally:
        setter(old)


def _ld(t):
    return t.stride(0) if t.dim() == 2 else t.shape[-1]


def _gemm8_try(a, b, c, aux, bias, src, m, n, k, a_kc, b_kc, act, splitk=1, accumulate=False, alpha=1.0):
    fn = _proto("dle_gemm8_try", _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _LL, _I, _I, _I, _I, _I, _I, _I, _FL, _VP, _VP,
                _VP)
    return fn(C.ptr(a), C.ptr(b), C.ptr(c), C.ptr(aux), C.ptr(bias), C.ptr(src), m, n, k, _ld(a), _ld(b), _ld(c), int(a_kc), int(b_kc),
              C.dt(a), C.dt(c), act, splitk, int(accumulate), alpha, None, None, C.stream())


def _dma_try(a, b, c, aux, bias, src, m, n, k, a_kc, b_kc, act, splitk=1, accumulate=False, alpha=1.0):
    fn = _proto("dle_gemm_dma_try", _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _LL, _I, _I, _I, _I, _I, _I, _I, _FL, _VP,
                _LL, _VP)
    ws = F.splitk_workspace(a.device, splitk * m * n * 4) if splitk > 1 else None
    return fn(C.ptr(a), C.ptr(b), C.ptr(c), C.ptr(aux), C.ptr(bias), C.ptr(src), m, n, k, _ld(a), _ld(b), _ld(c), int(a_kc), int(b_kc),
              C.dt(a), C.dt(c), act, splitk, int(accumulate), alpha, C.ptr(ws), ws.numel() * 4 if ws is not None else 0, C.stream())


def _smallm_try(a, b, c, bias, src, m, n, k, act_add, accumulate, alpha):
    fn = _proto("dle_gemm_smallm_try", _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _LL, _I, _I, _I, _I, _FL, _VP)
    return fn(C.ptr(a), C.ptr(b), C.ptr(c), C.ptr(bias), C.ptr(src), m, n, k, _ld(a), _ld(b), _ld(c), C.dt(a), C.dt(c), int(act_add),
              int(accumulate), alpha, C.stream())


def _expand_try(a, b, c, src, keep, m, n, k, b_kc, act):
    fn = _proto("dle_gemm_expand_try", _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _LL, _I, _I, _I, _I, _VP)
    return fn(C.ptr(a), C.ptr(b), C.ptr(c), C.ptr(src), C.ptr(keep), None, m, n, k, _ld(a), _ld(b), _ld(c), int(b_kc), C.dt(a), C.dt(c),
              {C.ACT_NONE: 0, C.ACT_ADD: 1, C.ACT_ADD_MASKED: 2}[act], C.stream())


# ---------------------------------------------------------------- one F.gemm case
EPI = {  # name -> (act, bias, source tensor, side output)
    "none": (C.ACT_NONE, False, False, False), "bias": (C.ACT_NONE, True, False, False),
    "bias_relu": (C.ACT_RELU, True, False, False), "bias_gelu_pre": (C.ACT_GELU, True, False, True),
    "bias_gelu_daux": (C.ACT_GELU_DAUX, True, False, True), "bias_tanh": (C.ACT_TANH, True, False, False),
    "relu_bwd": (C.ACT_RELU_BWD, False, True, False), "add": (C.ACT_ADD, False, True, False),
    "add_masked": (C.ACT_ADD_MASKED, False, True, False), "mul": (C.ACT_MUL, False, True, False),
    "tanh_bwd": (C.ACT_TANH_BWD, False, True, False), "gelu_bwd": (C.ACT_GELU_BWD, False, True, False)}
TRANSCENDENTAL = ("bias_gelu_pre", "bias_gelu_daux", "bias_tanh", "gelu_bwd")


class Case:
    def __init__(self, cid, site, m, n, k, layout, epi="none", f32=False, splitk=1, route="g8", accumulate=(False,), alpha=1.0,
                 pad_a=0, pad_c=0, offset_a=0, twice=True):
        self.cid, self.site, self.m, self.n, self.k, self.layout, self.epi = cid, site, m, n, k, layout, epi
        self.f32, self.splitk, self.route, self.accumulate, self.alpha = f32, splitk, route, accumulate, alpha
        self.pad_a, self.pad_c, self.offset_a, self.twice = pad_a, pad_c, offset_a, twice


def _strided(t, pad, offset=0):
    """The same values as a row-strided view (pitch + pad, first column `offset`) of a wider buffer."""
    if not pad and not offset:
        return t
    wide = torch.zeros((t.shape[0], t.shape[1] + pad + offset), dtype=t.dtype, device=t.device)
    v = wide[:, offset:offset + t.shape[1]]
    v.copy_(t)
    return v


class _Out2d:
    """Out for a row-strided [m, n] view of a NaN-filled [m, n + pad] buffer: the pad columns and the tail keep their bits."""

    def __init__(self, m, n, pad, dtype, dev, fill=None):
        self.o = Out((m, n + pad), dtype, dev)
        self.t = self.o.t[:, :n]
        if fill is not None:
            self.t.copy_(fill)
        self.pad = _bits(self.o.t[:, n:]).clone() if pad else None
        self.n = n

    def check(self, what):
        self.o.check(what)
        if self.pad is not None:
            assert torch.equal(_bits(self.o.t[:, self.n:]), self.pad), "%s wrote between the rows of its output" % what
        return self.t


def _run_case(dev, dtype, c):
    m, n, k, layout = c.m, c.n, c.k, c.layout
    a_kc, b_kc = layout != "tn", layout == "nt"
    act, has_bias, has_src, has_aux = EPI[c.epi]
    thin = dict(kmax=1, density=0.25) if c.epi in TRANSCENDENTAL else {}
    sa, sb = _shapes(layout, m, n, k)
    sd = _seed(c.cid, DT_IDS[dtype])
    a = _strided(grid(sa, sd, dtype, dev, kmax=1 if thin else 4), c.pad_a, c.offset_a)
    b = grid(sb, sd + 1, dtype, dev, **thin)
    bias = grid((n,), sd + 2, F32, dev, kmax=8) * 0.25 if has_bias else None             # multiples of 1/16
    src = _strided(grid((m, n), sd + 3, dtype, dev), c.pad_c) if has_src else None      # the epilogues read it with C's row pitch
    keep = torch.rand((m, n), generator=gen(dev, sd + 4), device=dev) < 0.6 if c.epi == "add_masked" else None
    keep_bits = _pack_bits(keep) if keep is not None else None
    out_dtype = F32 if c.f32 else dtype
    splitk = F.pick_splitk(m, n, k, c.splitk[1]) if isinstance(c.splitk, tuple) else c.splitk

    # ---- reference and its exactness precondition, from the data
    pre = c.alpha * _prod64(layout, a, b)
    mag = abs(c.alpha) * _prod64(layout, a.abs(), b.abs())
    del_scale = 16.0 / min(c.alpha, 1.0)
    if has_bias:
        pre, mag = pre + bias.to(F64), mag + bias.to(F64).abs()
    e_main = e_aux = None
    want_aux = None
    if c.epi in ("none", "bias"):
        ref = pre
    elif c.epi == "bias_relu":
        ref = pre.clamp_min(0)
    elif c.epi == "relu_bwd":
        ref = torch.where(src.to(F64) > 0, pre, torch.zeros_like(pre))
    elif c.epi == "add":
        ref, mag = pre + src.to(F64), mag + src.to(F64).abs()
    elif c.epi == "add_masked":
        s64 = torch.where(keep, src.to(F64), torch.zeros_like(pre))
        ref, mag = pre + s64, mag + s64.abs()
    elif c.epi == "mul":
        ref, del_scale = pre * src.to(F64), 64.0
    elif c.epi == "tanh_bwd":
        y = src.to(F64)
        assert float(y.abs().max()) <= 1.0
        ref, del_scale = pre * (1 - y * y), 256.0
    elif c.epi == "bias_tanh":
        ref = torch.tanh(pre)
        e_main = _tanh_err(pre, ref) * SECOND_ORDER
    elif c.epi == "bias_gelu_pre":
        ref, e_main, _, _ = _gelu64(pre)
        want_aux = pre.float().to(dtype)
    elif c.epi == "bias_gelu_daux":
        ref, e_main, ref_aux, e_aux = _gelu64(pre)
    else:                                                                                   # gelu_bwd: src = the pre-activation
        _, _, d, ed = _gelu64(src.to(F64))
        ref = pre * d
        e_main = (pre.abs() * ed + U * ref.abs()) * SECOND_ORDER
    worst = float(mag.max())
    assert worst < B_MFMA, "%s: sum of magnitudes up to %g: fp32 sums would not be exact" % (c.cid, worst)
    assert torch.equal(pre * del_scale, torch.round(pre * del_scale)), "%s: a term off the grid" % c.cid
    if c.f32:
        assert worst * del_scale < 2.0 ** 24, "%s: an fp32 output would not hold its value" % c.cid
    del mag
    want = ref.float().to(out_dtype) if e_main is None else None
    what = "%s [%s] %dx%dx%d %s %s" % (c.cid, c.site, m, n, k, layout, c.epi)
    aux_arg = lambda o: keep_bits if keep_bits is not None else (o.t if o is not None else None)

    for accumulate in c.accumulate:
        dw0 = grid((m, n), sd + 5, F32, dev) if accumulate else None
        if accumulate:
            assert float((_prod64(layout, a.abs(), b.abs()) + dw0.to(F64).abs()).max()) < B_MFMA
            want = (ref + dw0.to(F64)).float()
        elif e_main is None:
            want = ref.float().to(out_dtype)

        def fresh():
            return (_Out2d(m, n, c.pad_c, out_dtype, dev, fill=dw0), Out((m, n), dtype, dev) if has_aux else None)

        def compare(o, oa, who):
            got = o.check(who + " " + what)
            if e_main is None:
                assert_same(got, want, who + " " + what)
            else:
                _assert_within(got, ref, e_main, who + " " + what)
            if oa is not None:
                ga = oa.check(who + " side output " + what)
                if want_aux is not None:
                    assert_same(ga, want_aux, who + " pre-activation " + what)
                else:
                    _assert_within(ga, ref_aux, e_aux, who + " gelu' " + what)

        def wrapper(o, oa):
            F.gemm(a, b, m, n, k, a_kc, b_kc, out=o.t, bias=bias, act=act, aux=aux_arg(oa), mask_src=src, splitk=splitk,
                   accumulate=accumulate, alpha=c.alpha)

        # ---- the kernel the case belongs to, through its own entry point
        o, oa = fresh()
        n0 = _count()
        if c.route == "g8" and splitk == 1:
            rc = _gemm8_try(a, b, o.t, aux_arg(oa), bias, src, m, n, k, a_kc, b_kc, act, 1, accumulate, c.alpha)
            took = rc == 1 and _count() - n0 == 1
        elif c.route in ("g8", "dma"):
            rc = _dma_try(a, b, o.t, aux_arg(oa), bias, src, m, n, k, a_kc, b_kc, act, splitk, accumulate, c.alpha)
            took = rc == 1 and _count() - n0 == (1 if c.route == "g8" else 0)
        elif c.route == "smallm":
            rc = _smallm_try(a, b, o.t, bias, src, m, n, k, act == C.ACT_ADD, accumulate, c.alpha)
            took = rc == 1
        elif c.route == "expand":
            rc = _expand_try(a, b, o.t, src, keep_bits, m, n, k, b_kc, act)
            took = rc == 1
        else:                                                                               # legacy: gemm_dma.hip must decline
            rc = _dma_try(a, b, o.t, aux_arg(oa), bias, src, m, n, k, a_kc, b_kc, act, splitk, accumulate, c.alpha)
            took = rc == 0
        assert rc in (0, 1), "%s: entry point of route %s failed with %d" % (what, c.route, rc)
        if took and c.route != "legacy":
            compare(o, oa, c.route)
        # ---- the public wrapper: the same bits, the same kernel
        o, oa = fresh()
        n0 = _count()
        wrapper(o, oa)
        moved = _count() - n0
        compare(o, oa, "F.gemm")
        assert took, "%s: the launch did not go to %s (return code %d, ping-pong launches %d)" % (what, c.route, rc, moved)
        assert moved == (1 if c.route == "g8" else 0), "%s: F.gemm ran %d ping-pong launches, route %s" % (what, moved, c.route)
        # ---- the tile kernels at the same size
        if c.twice:
            with _pinned_off():
                o, oa = fresh()
                n0 = _count()
                wrapper(o, oa)
                assert _count() == n0, "%s: dle_gemm8_mode(0) did not pin the ping-pong kernel off" % what
                compare(o, oa, "F.gemm (ping-pong off)")


E, P = "bert/engine.py", "dlrm/model.py"
BERT = [
    # forward, both operands K-contiguous
    Case("qkv", E + ":240", T, 3 * H, H, "nt", "bias"),
    Case("attn_out", E + ":264", T, H, H, "nt", "bias"),
    Case("ffn1", E + ":274", T, I, H, "nt", "bias_gelu_daux"),
    Case("ffn2", E + ":276", T, H, I, "nt", "bias"),
    Case("pooler", E + ":289", B, H, H, "nt", "bias_tanh", route="dma"),
    Case("nsp", E + ":291", B, 8, H, "nt", "bias", f32=True, route="smallm"),
    Case("mlm_transform", E + ":297", NM, H, H, "nt", "bias_gelu_pre", route="dma"),
    Case("mlm_logits", E + ":300", NM, V, H, "nt", "bias", f32=True),
    # data gradients, B stored [k][n]
    Case("d_mlm_logits", E + ":373", NM, H, V, "nn", route="dma"),
    Case("d_mlm_transform", E + ":381", NM, H, H, "nn", route="dma"),
    Case("d_nsp", E + ":398", B, H, 8, "nn", "tanh_bwd", route="dma"),
    Case("d_pooler", E + ":401", B, H, H, "nn", route="dma"),
    Case("d_ffn2_mul", E + ":429", T, I, H, "nn", "mul"),
    Case("d_ffn1", E + ":434", T, H, I, "nn", "add"),
    Case("d_attn_out", E + ":449", T, H, H, "nn"),
    Case("d_qkv", E + ":479", T, H, 3 * H, "nn", "add"),
    # weight gradients, both M / N-contiguous, fp32, the engine's split (_wgrad, bert/engine.py:356-357)
    Case("w_mlm_decoder", E + ":371", V, H, NM, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
    Case("w_mlm_transform", E + ":379", H, H, NM, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
    Case("w_nsp", E + ":386", 8, H, B, "tn", f32=True, route="dma"),
    Case("w_pooler", E + ":399", H, H, B, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True), route="dma"),
    Case("w_ffn2", E + ":422", H, I, T, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
    Case("w_ffn1", E + ":431", I, H, T, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
    Case("w_attn_out", E + ":448", H, H, T, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
    Case("w_qkv", E + ":477", 3 * H, H, T, "tn", f32=True, splitk=("pick", 1024), accumulate=(False, True)),
]
DLRM = [
    # forward layers gemm_relu_bits does not take (K = 16 is below the ping-pong kernel's two K tiles; the last layer of each MLP)
    Case("bot0", P + ":122", MD, 512, 16, "nt", "bias_relu", route="dma"),
    Case("bot2", P + ":122", MD, 128, 256, "nt", "bias_relu", route="dma"),
    Case("top3", P + ":122", MD, 256, 512, "nt", "bias_relu"),
    # the fallback of the masked data gradients, and the input gradient of the top MLP
    Case("d_top1_relu", P + ":185", MD, 1024, 1024, "nn", "relu_bwd"),
    Case("d_bot2_relu", P + ":185", MD, 256, 128, "nn", "relu_bwd"),
    Case("d_top0", P + ":189", MD, 480, 1024, "nn"),
    # weight gradients over 65,536 rows, pick_splitk's default target (dlrm/model.py:152-153)
    Case("w_bot0", P + ":152", 512, 16, MD, "tn", f32=True, splitk=("pick", 512), route="dma"),
    Case("w_bot1", P + ":152", 256, 512, MD, "tn", f32=True, splitk=("pick", 512)),
    Case("w_bot2", P + ":152", 128, 256, MD, "tn", f32=True, splitk=("pick", 512), route="dma"),
    Case("w_top0", P + ":152", 1024, 480, MD, "tn", f32=True, splitk=("pick", 512)),
    Case("w_top1", P + ":152", 1024, 1024, MD, "tn", f32=True, splitk=("pick", 512)),
    Case("w_top2", P + ":152", 512, 1024, MD, "tn", f32=True, splitk=("pick", 512)),
    Case("w_top3", P + ":152", 256, 512, MD, "tn", f32=True, splitk=("pick", 512)),
]
# ragged shapes, one per route: prime M, N off the 128 / 256 tiles, a K tail of 8, row-strided A and C
RAGGED = [
    Case("g8_nt", "ragged", 8209, 1304, 328, "nt", "bias_relu", pad_a=24, pad_c=16),
    Case("g8_nn_masked", "ragged", 4096, 2048, 512, "nn", "add_masked"),
    Case("g8_4096x2560x256", "tests/test_gpu_gemm.py BIG_CASES", 4096, 2560, 256, "nt", "bias_relu"),
    Case("g8_tn_split", "ragged", 1032, 776, 4160, "tn", f32=True, splitk=9, accumulate=(False, True)),
    Case("dma_nn", "ragged", 1009, 200, 136, "nn", "add", route="dma", pad_a=8, pad_c=8),
    Case("dma_nn_masked", "ragged", 1009, 200, 136, "nn", "add_masked", route="dma"),
    Case("dma_nn_gelu_bwd", "ragged", 1009, 200, 136, "nn", "gelu_bwd", route="dma"),
    Case("dma_tn_split", "ragged", 200, 136, 968, "tn", f32=True, splitk=3, accumulate=(False, True), route="dma", pad_c=4),
    Case("legacy_nt", "ragged", 300, 72, 128, "nt", "bias_relu", route="legacy", pad_a=162, offset_a=10, twice=False),
    Case("legacy_nt_atomics", "ragged", 300, 72, 136, "nt", f32=True, splitk=3, accumulate=(False, True), route="legacy", pad_a=154,
         offset_a=10, twice=False),
    Case("expand_nn_add", "ragged", 4101, 256, 64, "nn", "add", route="expand"),
    Case("expand_nt_masked", "ragged", 4101, 512, 128, "nt", "add_masked", route="expand"),
    Case("smallm_alpha_acc", "ragged", 200, 72, 264, "nt", "bias", f32=True, route="smallm", alpha=0.5, accumulate=(False, True),
         pad_a=24, pad_c=12, twice=False),
    Case("smallm_add", "ragged", 129, 36, 136, "nt", "add", route="smallm", twice=False),
]


def test_source_pitch_is_checked(cuda):
    """The source-tensor epilogues address mask_src with the output's row pitch: F.gemm refuses another one (a dense source behind
    a row-strided output would be read past its end)."""
    a, b = grid((64, 64), 1, HF, cuda), grid((64, 32), 2, HF, cuda)
    src, wide = grid((64, 32), 3, HF, cuda), torch.zeros((64, 40), dtype=HF, device=cuda)
    with pytest.raises(ValueError, match="row pitch"):
        F.gemm(a, b, 64, 32, 64, True, False, out=wide[:, :32], act=C.ACT_ADD, mask_src=src)


def _params(cases):
    return [pytest.param(c, dt, id="%s-%s" % (c.cid, DT_IDS[dt])) for c in cases for dt in (BF, HF)]


@pytest.mark.parametrize("case, dtype", _params(BERT))
def test_bert_large_gemm(cuda, case, dtype):
    """Every F.gemm launch of the BERT-Large step at batch 256 x 128 (the site is the call's line)."""
    _run_case(cuda, dtype, case)


@pytest.mark.parametrize("case, dtype", _params(DLRM))
def test_dlrm_gemm(cuda, case, dtype):
    """The F.gemm launches of the DLRM MLPs at 65,536 rows; K = 480 is 7.5 K tiles, K = 16 a quarter of one."""
    _run_case(cuda, dtype, case)


@pytest.mark.parametrize("case, dtype", _params(RAGGED))
def test_ragged_gemm(cuda, case, dtype, monkeypatch):
    if case.cid in ("g8_nt", "dma_nn"):
        assert all(case.m % q for q in range(2, 91)), "M is meant to be prime"
    _run_case(cuda, dtype, case)
    if case.route == "expand":                     # DLE_GEMM_EXPAND is read per call: the tile kernel at the same shape
        monkeypatch.setenv("DLE_GEMM_EXPAND", "0")
        pinned = Case(case.cid + "_tile", case.site, case.m, case.n, case.k, case.layout, case.epi, route="dma", twice=False)
        pinned.cid = case.cid                      # the same inputs
        _run_case(cuda, dtype, pinned)


# ================================================================ gemm_relu_bits, gemm_colsum, gemm_colsum_bits
def _thin(shape, seed, dtype, dev):
    return grid(shape, seed, dtype, dev, kmax=2, density=0.5)


def _colsum_exact(dx64, scale, cs0=None):
    """The column sums of the stored dX are exact in fp32: terms multiples of 1 / scale, column magnitude sums x scale < 2^24."""
    assert torch.equal(dx64 * scale, torch.round(dx64 * scale)), "a stored gradient off the grid"
    worst = dx64.abs().sum(0) + (cs0.to(F64).abs() if cs0 is not None else 0)
    assert float(worst.max()) * scale < 2.0 ** 24, "column magnitude sum %g: fp32 column sums would not be exact" % float(worst.max())


RELU_BITS = [("bot0", 512, 16, 0), ("bot1", 256, 512, 1), ("top0", 1024, 480, 1), ("top1", 1024, 1024, 1), ("top2", 512, 1024, 1)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("lid, n, k, rc", RELU_BITS, ids=[r[0] for r in RELU_BITS])
def test_dlrm_relu_bits(cuda, lid, n, k, rc, dtype):
    """dlrm/model.py:118, gemm_relu_bits at 65,536 rows: y bit-exact, bits = ref64 > 0; K = 16 declines (model.py:122 takes it:
    test_dlrm_gemm bot0)."""
    m, sd = MD, _seed("relu_bits", lid, DT_IDS[dtype])
    x, w = grid((m, k), sd, dtype, cuda), grid((n, k), sd + 1, dtype, cuda)
    bias = grid((n,), sd + 2, F32, cuda, kmax=8) * 0.25
    pre = x.to(F64) @ w.to(F64).t() + bias.to(F64)
    assert float((x.to(F64).abs() @ w.to(F64).abs().t() + bias.to(F64).abs()).max()) < B_MFMA
    assert torch.equal(pre * 16, torch.round(pre * 16))
    want, want_bits = pre.clamp_min(0).float().to(dtype), _pack_bits(pre > 0)
    fn = _proto("dle_gemm8_relu_bits_try", _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _I, _VP)
    oy, ob = Out((m, n), dtype, cuda), Out((m * n // 8,), torch.uint8, cuda)
    n0 = _count()
    assert fn(C.ptr(x), C.ptr(w), C.ptr(oy.t), C.ptr(ob.t), C.ptr(bias), m, n, k, k, k, C.dt(x), C.stream()) == rc
    r = F.gemm_relu_bits(x, w, m, n, k, bias)
    if rc == 0:
        assert r is None and _count() == n0
        return
    assert _count() - n0 == 2
    assert_same(oy.check("relu_bits y"), want, "gemm8_relu_bits_try y " + lid)
    assert_same(ob.check("relu_bits bits"), want_bits, "gemm8_relu_bits_try bits " + lid)
    assert_same(r[0], want, "gemm_relu_bits y " + lid)
    assert_same(r[1], want_bits, "gemm_relu_bits bits " + lid)
    with _pinned_off():
        assert F.gemm_relu_bits(x, w, m, n, k, bias) is None


# (site, m, n, k, act): dX [m, n] = f(g [m, k] w [k, n], src) + column sums
COLSUM = [("ffn2", E + ":424", T, I, H, C.ACT_MUL), ("top1", P + ":180", MD, 1024, 1024, C.ACT_RELU_BWD),
          ("bot2", P + ":180", MD, 256, 128, C.ACT_RELU_BWD), ("ragged", "ragged", 1009, 200, 136, C.ACT_RELU_BWD)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cid, site, m, n, k, act", COLSUM, ids=[c[0] for c in COLSUM])
def test_gemm_colsum(cuda, cid, site, m, n, k, act, dtype):
    """gemm_colsum: dX and the column sums of the STORED dX bit for bit, accumulate=True included; ping-pong kernel (256 | M) and,
    pinned off, the tile kernels' statistics epilogue."""
    sd = _seed("colsum", cid, DT_IDS[dtype])
    g, w = _thin((m, k), sd, dtype, cuda), _thin((k, n), sd + 1, dtype, cuda)
    src = grid((m, n), sd + 2, dtype, cuda)
    prod = g.to(F64) @ w.to(F64)
    assert float((g.to(F64).abs() @ w.to(F64).abs()).max()) < B_MFMA
    if act == C.ACT_MUL:
        ref, scale = prod * src.to(F64), 64.0
    else:
        ref, scale = torch.where(src.to(F64) > 0, prod, torch.zeros_like(prod)), 16.0
    assert torch.equal(ref * scale, torch.round(ref * scale))
    want = ref.float().to(dtype)
    cs0 = grid((n,), sd + 3, F32, cuda)
    _colsum_exact(want.to(F64), scale, cs0)
    want_cs = want.to(F64).sum(0)
    what = "gemm_colsum %s [%s] %dx%dx%d" % (cid, site, m, n, k)
    g8 = m % 256 == 0 and m >= 256 and n >= 256 and k >= 128
    fn = _proto("dle_gemm_colsum", _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _LL, _I, _I, _I, _VP, _LL, _VP)
    for pinned in (False, True):
        with (_pinned_off() if pinned else contextlib.nullcontext()):
            for accumulate in (False, True):
                od, oc = Out((m, n), dtype, cuda), Out((n,), F32, cuda, fill=cs0 if accumulate else None)
                ws = F.splitk_workspace(cuda, ((m + 127) // 128) * n * 4)
                n0 = _count()
                rc = fn(C.ptr(g), C.ptr(w), C.ptr(od.t), C.ptr(src), C.ptr(oc.t), m, n, k, k, n, n, C.dt(g), act, int(accumulate),
                        C.ptr(ws), ws.numel() * 4, C.stream())
                assert rc == 1, "%s: dle_gemm_colsum returned %d" % (what, rc)
                assert _count() - n0 == (1 if g8 and not pinned else 0), "%s: ping-pong launches %d" % (what, _count() - n0)
                assert_same(od.check(what), want, what + " dX")
                assert_same(oc.check(what), (want_cs + (cs0.to(F64) if accumulate else 0)).float(),
                            what + " column sums, accumulate=%s pinned=%s" % (accumulate, pinned))
            cs = cs0.clone()
            dx = F.gemm_colsum(g, w, m, n, k, src, cs, act=act, accumulate=True)
            assert dx is not None
            assert_same(dx, want, what + " wrapper dX")
            assert_same(cs, (want_cs + cs0.to(F64)).float(), what + " wrapper column sums")


COLSUM_BITS = [("top3", 512, 256), ("top2", 1024, 512), ("top1", 1024, 1024), ("bot2", 256, 128), ("bot1", 512, 256)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("lid, n, k", COLSUM_BITS, ids=[c[0] + "-%dx%d" % c[1:] for c in COLSUM_BITS])
def test_dlrm_colsum_bits(cuda, lid, n, k, dtype):
    """dlrm/model.py:178, gemm_colsum_bits at 65,536 rows with random keep bits: dX and column sums bit for bit."""
    m, sd = MD, _seed("colsum_bits", lid, n, k, DT_IDS[dtype])
    g, w = _thin((m, k), sd, dtype, cuda), _thin((k, n), sd + 1, dtype, cuda)
    keep = torch.rand((m, n), generator=gen(cuda, sd + 2), device=cuda) < 0.5
    kb = _pack_bits(keep)
    prod = g.to(F64) @ w.to(F64)
    assert float((g.to(F64).abs() @ w.to(F64).abs()).max()) < B_MFMA
    assert torch.equal(prod * 16, torch.round(prod * 16))
    want = torch.where(keep, prod, torch.zeros_like(prod)).float().to(dtype)
    cs0 = grid((n,), sd + 3, F32, cuda)
    _colsum_exact(want.to(F64), 16.0, cs0)
    want_cs = want.to(F64).sum(0)
    what = "gemm_colsum_bits %s %dx%dx%d" % (lid, m, n, k)
    fn = _proto("dle_gemm_colsum_bits", _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _LL, _LL, _I, _I, _VP, _LL, _VP)
    for accumulate in (False, True):
        od, oc = Out((m, n), dtype, cuda), Out((n,), F32, cuda, fill=cs0 if accumulate else None)
        ws = F.splitk_workspace(cuda, ((m + 127) // 128) * n * 4)
        n0 = _count()
        rc = fn(C.ptr(g), C.ptr(w), C.ptr(od.t), C.ptr(kb), C.ptr(oc.t), m, n, k, k, n, C.dt(g), int(accumulate), C.ptr(ws),
                ws.numel() * 4, C.stream())
        assert rc == 1 and _count() - n0 == 1, "%s: return code %d, ping-pong launches %d" % (what, rc, _count() - n0)
        assert_same(od.check(what), want, what + " dX")
        assert_same(oc.check(what), (want_cs + (cs0.to(F64) if accumulate else 0)).float(), what + " column sums")
    cs = cs0.clone()
    dx = F.gemm_colsum_bits(g, w, m, n, k, kb, cs, accumulate=True)
    assert dx is not None
    assert_same(dx, want, what + " wrapper dX")
    assert_same(cs, (want_cs + cs0.to(F64)).float(), what + " wrapper column sums")
    with _pinned_off():
        assert F.gemm_colsum_bits(g, w, m, n, k, kb, cs) is None


# ================================================================ gemm_batched: the unfused attention path
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_bert_large_gemm_batched(cuda, dtype):
    """The six gemm_batched calls of bert/engine.py:253-263 and :458-470 at b x heads = 4096 batches, s = 128, d = 64, with the
    engine's strides into the packed QKV buffer, against a float64 einsum over the same views; the columns of the packed dqkv a
    call does not own keep their bits."""
    b, s, h, nh = B, 128, H, 16
    d, t = h // nh, B * 128
    sd = _seed("batched", DT_IDS[dtype])
    qkv = grid((t, 3 * h), sd, dtype, cuda)
    dctx = grid((t, h), sd + 1, dtype, cuda)
    pdrop = grid((b * nh, s, s), sd + 2, dtype, cuda)
    dprobs_in = grid((b * nh, s, s), sd + 3, dtype, cuda)
    heads = lambda x2d: x2d.to(F64).view(b, s, nh, d)                                  # [t, h] columns -> [b, s, head, d]
    q, k, v, do = heads(qkv[:, :h]), heads(qkv[:, h:2 * h]), heads(qkv[:, 2 * h:]), heads(dctx)
    p64, ds64 = pdrop.to(F64).view(b, nh, s, s), dprobs_in.to(F64).view(b, nh, s, s)
    biggest = max(float(x.abs().max()) for x in (qkv, dctx, pdrop, dprobs_in))
    assert max(d, s) * biggest * biggest < B_MFMA, "sum of magnitudes: fp32 sums would not be exact"
    sp, sq, sc = (nh * s * s, s * s), (s * 3 * h, d), (s * h, d)

    def same(got, ref, what):
        assert torch.equal(ref * 16, torch.round(ref * 16))
        assert_same(got, ref.float().to(dtype), "gemm_batched " + what)

    probs = Out((b * nh, s, s), dtype, cuda)                                            # engine.py:253  Q K^T
    F.gemm_batched(qkv, qkv[:, h:], probs.t, s, s, d, 3 * h, 3 * h, s, True, True, b * nh, nh, sq, sq, sp)
    same(probs.check("QK^T").view(b, nh, s, s), torch.einsum("bihd,bjhd->bhij", q, k), "Q K^T")
    del probs
    ctx = Out((t, h), dtype, cuda)                                                      # engine.py:262  P V
    F.gemm_batched(pdrop, qkv[:, 2 * h:], ctx.t, s, d, s, s, 3 * h, h, True, False, b * nh, nh, sp, sq, sc)
    same(ctx.check("PV").view(b, s, nh, d), torch.einsum("bhij,bjhd->bihd", p64, v), "P V")
    del ctx
    dprobs = Out((b * nh, s, s), dtype, cuda)                                           # engine.py:458  dO V^T
    F.gemm_batched(dctx, qkv[:, 2 * h:], dprobs.t, s, s, d, h, 3 * h, s, True, True, b * nh, nh, sc, sq, sp)
    same(dprobs.check("dO V^T").view(b, nh, s, s), torch.einsum("bihd,bjhd->bhij", do, v), "dO V^T")
    del dprobs
    dqkv = Out((t, 3 * h), dtype, cuda)
    before = _bits(dqkv.t).clone()

    def others_untouched(lo, what):
        now = _bits(dqkv.check(what))
        assert torch.equal(now[:, :lo], before[:, :lo]) and torch.equal(now[:, lo + h:], before[:, lo + h:]), \
            "gemm_batched %s wrote outside its columns of dqkv" % what
        before[:, lo:lo + h] = now[:, lo:lo + h]

    F.gemm_batched(dprobs_in, qkv[:, h:], dqkv.t, s, d, s, s, 3 * h, 3 * h, True, False, b * nh, nh, sp, sq, sq)     # :465 dQ = dS K
    others_untouched(0, "dQ")
    same(dqkv.t[:, :h].reshape(b, s, nh, d), torch.einsum("bhij,bjhd->bihd", ds64, k), "dQ = dS K")
    F.gemm_batched(dprobs_in, qkv, dqkv.t[:, h:], s, d, s, s, 3 * h, 3 * h, False, False, b * nh, nh, sp, sq, sq)     # :467 dK = dS^T Q
    others_untouched(h, "dK")
    same(dqkv.t[:, h:2 * h].reshape(b, s, nh, d), torch.einsum("bhij,bihd->bjhd", ds64, q), "dK = dS^T Q")
    F.gemm_batched(pdrop, dctx, dqkv.t[:, 2 * h:], s, d, s, s, h, 3 * h, False, False, b * nh, nh, sp, sc, sq)        # :469 dV = P^T dO
    others_untouched(2 * h, "dV")
    same(dqkv.t[:, 2 * h:].reshape(b, s, nh, d), torch.einsum("bhij,bihd->bjhd", p64, do), "dV = P^T dO")


# ================================================================ realistic inputs
def _gamma(n):
    return n * U / (1 - n * U)


def _gauss(shape, seed, dtype, dev, scale=1.0):
    return (torch.randn(shape, generator=gen(dev, seed), device=dev) * scale).to(dtype)


GAUSS = [("bert_ffn", "nt", T, I, H), ("bert_ffn", "nn", T, H, I), ("bert_ffn", "tn", I, H, T),
         ("dlrm_top0", "nt", MD, 1024, 480), ("dlrm_top0", "nn", MD, 480, 1024), ("dlrm_top0", "tn", 1024, 480, MD)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("gid, layout, m, n, k", GAUSS, ids=["%s-%s" % g[:2] for g in GAUSS])
def test_gaussian(cuda, gid, layout, m, n, k, dtype):
    """x ~ N(0, 1), w ~ N(0, 1 / K) (dy ~ N(0, 1 / 4) for the weight gradient): the error-analysis bars of the module docstring,
    ping-pong kernel and, pinned off, the tile kernels."""
    sd = _seed("gauss", gid, layout, DT_IDS[dtype])
    sa, sb = _shapes(layout, m, n, k)
    a = _gauss(sa, sd, dtype, cuda, 0.5 if layout == "tn" else 1.0)
    b = _gauss(sb, sd + 1, dtype, cuda, 1.0 if layout == "tn" else k ** -0.5)
    ref, absref = _prod64(layout, a, b), _prod64(layout, a.abs(), b.abs())
    target = 1024 if gid == "bert_ffn" else 512
    splitk = F.pick_splitk(m, n, k, target) if layout == "tn" else 1
    assert layout != "tn" or splitk > 1
    for pinned in (False, True):
        with (_pinned_off() if pinned else contextlib.nullcontext()):
            n0 = _count()
            got = F.gemm(a, b, m, n, k, layout != "tn", layout == "nt", out_dtype=F32 if layout == "tn" else dtype, splitk=splitk)
            assert _count() - n0 == (0 if pinned else 1)
            g = got.to(F64)
            d = (g - ref).abs()
            if layout == "tn":
                chain = -(-(-(-k // 64)) // splitk) * 64 + splitk + 16
                bar = _gamma(chain) * absref
            else:
                bar = 0.5 * ulp16(torch.maximum(g.abs(), ref.abs()), dtype) + _gamma(k + 2) * absref
            assert bool((d <= bar).all()), "%s %s pinned=%s: worst %g of the bar at %s" % (
                gid, layout, pinned, float((d / bar).max()), torch.nonzero(d > bar)[:4].tolist())
