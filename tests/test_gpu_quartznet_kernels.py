"""The three QuartzNet kernels (csrc/quartznet.hip) against float64, per element, nothing skipped.  GPU only.

dle_tcs_conv1d_packed_fwd -- contract (include/dle_mi355x.h), per output row p of sequence b:
    d[p,c]  = round16( sum_k dw[k,c] x[cu_in[b] + p stride + (k - ksize/2) dilation, c] )            (0 outside the sequence)
    y[p,ko] = round16( relu?( fmaf(scale[ko], sum_c pw[ko,c] d[p,c], shift[ko]) + residual[p,ko] ) )
checked in TWO STAGES through d_out, the d tile as the kernel feeds it to the matrix units:
  stage 1   |d_out - d64| <= ulp16(d64) / 2 + (ksize + 1) 2^-24 sum_k |dw x|
            (one rounding to the storage type + the fp32 error of a ksize-term fmaf chain);
  stage 2   with p64 the float64 pointwise product over the kernel's OWN d_out bits,
            |y - y64| <= ulp16(y64) / 2 + (C + 3) 2^-24 (|scale| sum_c |pw d| + |shift| + |residual|)
            (one rounding + a C-term fp32 sum, one fmaf, one addition).
Both bars are derived, not measured.  Reference: torch float64 on the GPU, per sequence over a zero-padded copy, one strided slice
per tap (no conv1d, nothing of this library).

Bit-exact cases (tests/_exact_grid.py).  x, pw, residual = k / 4 with |k| <= 4; dw = k / 4 on 8 taps (the first, the last and six
others) and zero elsewhere, so d is a sum of at most 8 multiples of 1/16 of magnitude <= 1: a multiple of 1/16 of magnitude <= 8, 8
significant bits, exact in bf16 and fp16 (asserted: d64 survives the round trip through the storage type).  The pointwise terms are
multiples of 1/64 with a magnitude sum <= 8 C <= 2^13 < B_MFMA: the fp32 accumulator is exact in any order.  scale is one of +-0.5,
+-1, +-2 and shift a multiple of 1/16: the value before the rounding is a multiple of 1/128 below 2^16 (asserted), exact in fp32, and
y is the float64 value rounded ONCE.

Tile sizes the cases are named after: the kernel takes tiles of T = 64 OUTPUT rows per sequence, 256 output channels per workgroup,
C in chunks of 64; a depthwise thread owns 8 rows and takes the taps in blocks of 8 (ksize is padded to a multiple of 8 with zero
taps).  The kernel is not persistent: there is no grid cap and no second trip, so no such case.
  conv1_s2   64 -> 256, k 33, stride 2, lens 37, 6, 1      odd and even lengths, a sequence shorter than the half-kernel
  b1         256 -> 256, k 33, lens 63, 64, 65, 129        T - 1, T, T + 1, 2 T + 1: the row-tile edges
  b2         256 -> 256, k 39, lens 80, 3
  b3_widen   256 -> 512, k 51, lens 70                     two channel blocks
  b4         512 -> 512, k 63, lens 70                     (63 taps: one zero tap of padding)
  b5         512 -> 512, k 75, lens 70, 1
  conv2_d2   512 -> 512, k 87, dilation 2, lens 100, 44, 1 the halo (86 rows) exceeds the sequence
  big_c      1024 -> 1024, k 3, lens 5                     the envelope's corner: 16 chunks, 4 channel blocks
  many_tiles 64 -> 64, k 3, 300 sequences of 65 rows       a grid of 604 workgroups, more than the device has CUs; 300 sequences
                                                           take five steps of the 64-sequence tile search
The chunk loop has two forms, with and without a register prefetch of the next chunk, which the launcher chooses by grid size.
run() forces each form in turn (F.tcs_prefetch_mode) for EVERY call of every test below -- every shape, type and epilogue, the
isolation and zero-length cases -- and compares the two outputs bit for bit before the result is checked; one more test runs a
small and a large grid under the default choice.
each with residual + ReLU, with neither, and with ReLU only (the ReLU cases assert that something was clipped).

Also: y is bit-identical with and without d_out (every random case); each sequence of b1 and conv2_d2 run alone equals, bit for
bit, its rows when packed between neighbours filled with +-1e4 (a halo leaking over a sequence boundary); a zero-length sequence in
the middle of a batch; an inf in one input row (the padding taps must not spread it); argument checks raise without a launch,
each matched on its message.

dle_qn_normalize_pack -- F = 64, lens (2, 3, 161, 1000), T_pad 1008, against float64.  The bar, with n frames, u = 2^-24, S =
max_t |x| of the feature, m / s the float64 mean / (std + 1e-5):
    mean:  a sum of n fp32 terms in any order and one division: |dm| <= (n + 1) u S
    std:   deviations carry dm and one rounding each; the sum of squares, the division by n - 1 and the square root add
           (n + 4) u relatively to the variance, half of that to the std: |ds| <= |dm| + (n + 6) u s
    value: v = (x - m) / s:  |dv| <= (2 u S + |dm|) / s + |v| (|ds| / s + 2 u)
    |got - v64| <= ulp16(v64) / 2 + 2 |dv|      (the factor 2 covers the second-order terms dropped above)
A feature with a constant value has std 0: the values are (x - mean) / 1e-5 with x - mean a rounding residue of the mean, exactly 0
when the constant is a power of two: asserted to be 0 there, as the reference gives.

dle_ctc_greedy_packed -- constructed logits: "a a _ a b b" -> "aab"; all blanks; length 1; length 0; a repeat across a sequence
boundary does not merge; an exact tie (the first maximum wins); n_classes 29 inside ld 32 with the padding columns at +1e30.  logp
against float64 log_softmax: |d| <= (n_classes + 8) 2^-24 (1 + |logp64|) + 2^-22: the fp32 subtraction, expf and logf (a few ulp each
at magnitudes <= 1 + |logp|) and an n_classes-term sum of values in (0, 1].
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from tests._exact_grid import B_MFMA, Out, assert_same, bits, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
F64 = torch.float64
DEV = "cuda"
T = 64

# name -> (C, Ko, ksize, stride, dilation, lens)
SHAPES = {
    "conv1_s2": (64, 256, 33, 2, 1, (37, 6, 1)),
    "b1": (256, 256, 33, 1, 1, (T - 1, T, T + 1, 2 * T + 1)),
    "b2": (256, 256, 39, 1, 1, (80, 3)),
    "b3_widen": (256, 512, 51, 1, 1, (70,)),
    "b4": (512, 512, 63, 1, 1, (70,)),
    "b5": (512, 512, 75, 1, 1, (70, 1)),
    "conv2_d2": (512, 512, 87, 1, 2, (100, 44, 1)),
    "big_c": (1024, 1024, 3, 1, 1, (5,)),
    "many_tiles": (64, 64, 3, 1, 1, (65,) * 300),
}
MODES = {"res_relu": (True, True), "plain": (False, False), "relu": (False, True)}


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32, device=DEV)


def out_lens(lens, stride):
    return [(n - 1) // stride + 1 if n > 0 else 0 for n in lens]


def ref_depthwise(x, dw, lens, stride, dilation):
    """(d64, mag) [total_out, C] float64: per sequence over a zero-padded copy, one strided slice per tap."""
    x, dw = x.to(F64), dw.to(F64)
    ks = dw.shape[0]
    halo = (ks // 2) * dilation
    ds, ms, start = [], [], 0
    for n in lens:
        seq = x[start:start + n]
        start += n
        if n == 0:
            continue
        ol = (n - 1) // stride + 1
        xp = torch.nn.functional.pad(seq, (0, 0, halo, halo))
        d = torch.zeros((ol, x.shape[1]), dtype=F64, device=x.device)
        m = torch.zeros_like(d)
        for k in range(ks):
            rows = xp[k * dilation:k * dilation + stride * (ol - 1) + 1:stride]
            d += dw[k] * rows
            m += (dw[k] * rows).abs()
        ds.append(d)
        ms.append(m)
    return torch.cat(ds), torch.cat(ms)


def run(x, dw, pw, scale, shift, lens, stride, dilation, residual, relu, want_d=True):
    ol = out_lens(lens, stride)
    total_out = sum(ol)
    cu_in = cu_of(lens)
    cu_out = cu_of(ol) if stride != 1 else None
    got = []
    before = F.tcs_prefetch_mode(-1)
    try:
        for form in (0, 1):                                  # EVERY call of every test runs both forms of the chunk loop
            F.tcs_prefetch_mode(form)
            oy = Out((total_out, pw.shape[0]), x.dtype, DEV)
            od = Out((total_out, x.shape[1]), x.dtype, DEV) if want_d else None
            y = F.tcs_conv1d_packed_fwd(x, dw, pw, scale, shift, cu_in, cu_out, total_out if stride != 1 else None, stride=stride,
                                        dilation=dilation, residual=residual, relu=relu, out=oy.t, d_out=od.t if want_d else None)
            assert y.data_ptr() == oy.t.data_ptr()
            torch.cuda.synchronize()
            got.append((oy.check("tcs_conv1d_packed_fwd y"), od.check("tcs_conv1d_packed_fwd d_out") if want_d else None))
    finally:
        F.tcs_prefetch_mode(before)
    assert_same(bits(got[1][0]), bits(got[0][0]), "y with and without the register prefetch")
    if want_d:
        assert_same(bits(got[1][1]), bits(got[0][1]), "d_out with and without the register prefetch")
    return got[0]


def signs(n, g):
    return (torch.randint(0, 2, (n,), generator=g, device=DEV) * 2 - 1).float()


@functools.lru_cache(maxsize=None)
def exact_case(name, dtype):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    total = sum(lens)
    x = grid((total, c), 11, dtype, DEV)
    g = gen(DEV, 13)
    taps = torch.zeros(ks, device=DEV)
    pick = torch.randperm(ks - 2, generator=g, device=DEV)[:6] + 1 if ks > 2 else torch.zeros(0, dtype=torch.long, device=DEV)
    taps[pick] = 1
    taps[0] = taps[ks - 1] = 1
    assert int(taps.sum()) <= 8
    dw = (grid((ks, c), 12, dtype, DEV).float() * taps[:, None]).to(dtype)
    pw = grid((ko, c), 14, dtype, DEV)
    scale = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (ko,), generator=g, device=DEV)] * signs(ko, g)
    shift = torch.randint(-64, 65, (ko,), generator=g, device=DEV).float() / 16
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    d64, _ = ref_depthwise(x, dw, lens, stride, dil)
    assert torch.equal(d64 * 16, torch.round(d64 * 16)) and float(d64.abs().max()) <= 8
    assert torch.equal(d64.float().to(dtype).double(), d64), "d is not exact in the storage type"
    mag = d64.abs() @ pw.double().abs().t()
    assert float(mag.max()) < B_MFMA
    acc = d64 @ pw.double().t()
    res = grid((d64.shape[0], ko), 15, dtype, DEV)
    return x, dw, pw, scale, shift, res, d64, acc


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_tcs_exact_grid_bits(name, dtype, mode):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    use_res, relu = MODES[mode]
    x, dw, pw, scale, shift, res, d64, acc = exact_case(name, dtype)
    pre = scale.double() * acc + shift.double()
    if use_res:
        pre = pre + res.double()
    assert torch.equal(pre * 128, torch.round(pre * 128)) and float(pre.abs().max()) < 2.0 ** 16
    want = pre
    if relu:
        assert bool((pre < 0).any()), "nothing for the ReLU to clip"
        want = pre.clamp_min(0)
    y, d = run(x, dw, pw, scale, shift, lens, stride, dil, res if use_res else None, relu)
    assert_same(bits(d), bits(d64.float().to(dtype)), "%s %s d_out" % (name, dtype))
    assert_same(bits(y), bits(want.float().to(dtype)), "%s %s %s y" % (name, dtype, mode))


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    total = sum(lens)
    g = gen(DEV, 21)
    x = torch.randn((total, c), generator=g, device=DEV).to(dtype)
    dw = (torch.randn((ks, c), generator=g, device=DEV) * ks ** -0.5).to(dtype)
    pw = (torch.randn((ko, c), generator=g, device=DEV) * c ** -0.5).to(dtype)
    scale = (torch.rand((ko,), generator=g, device=DEV) * 3.75 + 0.25) * signs(ko, g)
    shift = torch.randn((ko,), generator=g, device=DEV)
    res = torch.randn((sum(out_lens(lens, stride)), ko), generator=g, device=DEV).to(dtype)
    d64, dmag = ref_depthwise(x, dw, lens, stride, dil)
    return x, dw, pw, scale, shift, res, d64, dmag


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_tcs_random_inputs_two_stage_bars(name, dtype, mode):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    use_res, relu = MODES[mode]
    x, dw, pw, scale, shift, res, d64, dmag = random_case(name, dtype)
    r = res if use_res else None
    y, d = run(x, dw, pw, scale, shift, lens, stride, dil, r, relu)
    y2, _ = run(x, dw, pw, scale, shift, lens, stride, dil, r, relu, want_d=False)
    assert_same(bits(y2), bits(y), "%s: y with and without d_out" % name)
    # stage 1
    bar1 = ulp16(d64, dtype) / 2 + (ks + 1) * 2.0 ** -24 * dmag
    err1 = (d.double() - d64).abs()
    w1 = float((err1 / bar1).max())
    # stage 2, over the kernel's own d bits
    dk = d.double()
    p64 = dk @ pw.double().t()
    pmag = dk.abs() @ pw.double().abs().t()
    ref = scale.double() * p64 + shift.double()
    rmag = torch.zeros_like(ref)
    if use_res:
        ref = ref + res.double()
        rmag = res.double().abs()
    if relu:
        assert bool((ref < 0).any()), "nothing for the ReLU to clip"
        ref = ref.clamp_min(0)
    bar2 = ulp16(ref, dtype) / 2 + (c + 3) * 2.0 ** -24 * (scale.double().abs() * pmag + shift.double().abs() + rmag)
    err2 = (y.double() - ref).abs()
    w2 = float((err2 / bar2).max())
    print("%s %s %s: stage 1 max err / bar %.3f, stage 2 %.3f" % (name, dtype, mode, w1, w2))
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(y).all())
    assert bool((err1 <= bar1).all()), "%s d: %d of %d over the bar, worst ratio %.3f" % (name, int((err1 > bar1).sum()), err1.numel(), w1)
    assert bool((err2 <= bar2).all()), "%s y: %d of %d over the bar, worst ratio %.3f" % (name, int((err2 > bar2).sum()), err2.numel(), w2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["b1", "conv2_d2"])
def test_tcs_sequences_are_isolated(name, dtype):
    """Sequence i alone == its rows when every OTHER sequence of the batch holds +-1e4 (and the residual rows of the others too)."""
    c, ko, ks, stride, dil, lens = SHAPES[name]
    x, dw, pw, scale, shift, res, _, _ = random_case(name, dtype)
    g = gen(DEV, 31)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    for i, n in enumerate(lens):
        lo, hi = starts[i], starts[i + 1]
        loud = (signs(x.numel(), g).view_as(x) * 1e4).to(dtype)
        loud[lo:hi] = x[lo:hi]
        y_all, d_all = run(loud, dw, pw, scale, shift, lens, stride, dil, res, True)
        y_one, d_one = run(x[lo:hi].contiguous(), dw, pw, scale, shift, [n], stride, dil, res[lo:hi].contiguous(), True)
        assert_same(bits(d_all[lo:hi]), bits(d_one), "%s sequence %d d" % (name, i))
        assert_same(bits(y_all[lo:hi]), bits(y_one), "%s sequence %d y" % (name, i))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tcs_zero_length_sequence_mid_batch(dtype):
    c, ko, ks = 64, 64, 5
    g = gen(DEV, 41)
    lens_a, lens_b = [9, 0, 70, 0], [9, 70]
    x = torch.randn((79, c), generator=g, device=DEV).to(dtype)
    dw = (torch.randn((ks, c), generator=g, device=DEV) * 0.4).to(dtype)
    pw = (torch.randn((ko, c), generator=g, device=DEV) * 0.1).to(dtype)
    scale, shift = torch.ones(ko, device=DEV), torch.zeros(ko, device=DEV)
    for stride in (1, 2):
        ya, da = run(x, dw, pw, scale, shift, lens_a, stride, 1, None, False)
        yb, db = run(x, dw, pw, scale, shift, lens_b, stride, 1, None, False)
        assert_same(bits(ya), bits(yb), "zero-length y stride %d" % stride)
        assert_same(bits(da), bits(db), "zero-length d stride %d" % stride)
        assert bool(torch.isfinite(ya).all())


def test_tcs_prefetch_mode_and_the_choice_by_grid_size():
    """The switch answers the previous setting and defaults to 2 (by grid size); under the default a grid below the CU count (b1) and
    one above it (many_tiles, 604 workgroups) both equal the forced forms, which run() has already compared with each other."""
    assert F.tcs_prefetch_mode(-1) == 2
    assert F.tcs_prefetch_mode(0) == 2 and F.tcs_prefetch_mode(1) == 0 and F.tcs_prefetch_mode(7) == 1 and F.tcs_prefetch_mode(2) == 1
    assert F.tcs_prefetch_mode(-1) == 2
    for name in ("b1", "many_tiles"):
        c, ko, ks, stride, dil, lens = SHAPES[name]
        x, dw, pw, scale, shift, res, _, _ = random_case(name, BF)
        want, _ = run(x, dw, pw, scale, shift, lens, stride, dil, res, True)
        got = F.tcs_conv1d_packed_fwd(x, dw, pw, scale, shift, cu_of(lens), residual=res, relu=True)
        torch.cuda.synchronize()
        assert_same(bits(got), bits(want), "%s under the default choice" % name)


def test_tcs_padding_taps_leave_a_nonfinite_row_where_the_sum_has_it():
    """ksize 3 is padded to a block of 8 taps.  An inf at input row t belongs to output rows t - 1 .. t + 1 only; the padding taps
    are skipped, not multiplied by zero, so every other row stays finite (0 x inf would be NaN in rows t - 7 .. t - 2)."""
    c, t = 64, 40
    g = gen(DEV, 71)
    x = torch.randn((100, c), generator=g, device=DEV).to(HF)
    x[t, :] = float("inf")
    dw = (torch.rand((3, c), generator=g, device=DEV) + 0.5).to(HF)
    pw = torch.eye(c, device=DEV).to(HF)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y, d = run(x, dw, pw, sc, sh, [100], 1, 1, None, False)
    hit = torch.zeros(100, dtype=torch.bool, device=DEV)
    hit[t - 1:t + 2] = True
    assert bool(torch.isinf(d[hit]).all())
    assert bool(torch.isfinite(d[~hit]).all()) and bool(torch.isfinite(y[~hit]).all())


def test_tcs_argument_checks_raise_without_a_launch():
    c = 64
    x = torch.zeros((8, c), dtype=BF, device=DEV)
    dw = torch.zeros((3, c), dtype=BF, device=DEV)
    pw = torch.zeros((c, c), dtype=BF, device=DEV)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    cu = cu_of([8])
    F.tcs_conv1d_packed_fwd(x, dw, pw, sc, sh, cu)                                # the baseline call is inside the envelope
    with pytest.raises(ValueError, match="ksize must be odd"):                  # even ksize
        F.tcs_conv1d_packed_fwd(x, torch.zeros((4, c), dtype=BF, device=DEV), pw, sc, sh, cu)
    with pytest.raises(ValueError, match="not both 2"):                         # stride 2 with dilation 2
        F.tcs_conv1d_packed_fwd(x, dw, pw, sc, sh, cu, cu_of([4]), 4, stride=2, dilation=2)
    with pytest.raises(ValueError, match="C must be a multiple of 64"):         # C = 32
        F.tcs_conv1d_packed_fwd(torch.zeros((8, 32), dtype=BF, device=DEV), torch.zeros((3, 32), dtype=BF, device=DEV),
                                torch.zeros((c, 32), dtype=BF, device=DEV), sc, sh, cu)
    with pytest.raises(ValueError, match="16-bit activations and weights only"):  # fp32
        F.tcs_conv1d_packed_fwd(x.float(), dw.float(), pw.float(), sc, sh, cu)
    mis = torch.ones(c + 1, device=DEV)[1:]                                     # a misaligned operand
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    with pytest.raises(ValueError, match="16-byte aligned"):
        F.tcs_conv1d_packed_fwd(x, dw, pw, mis, sh, cu)
    with pytest.raises(ValueError, match="must not overlap"):                   # y aliasing x
        F.tcs_conv1d_packed_fwd(x, dw, pw, sc, sh, cu, out=x)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- normalize_pack
NORM_LENS = (2, 3, 161, 1000)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_pack_against_float64(dtype):
    f, t_pad, lens = 64, 1008, NORM_LENS
    g = gen(DEV, 51)
    x = torch.randn((len(lens), f, t_pad), generator=g, device=DEV) * 3 - 7          # log-mel-like: an offset larger than the spread
    x[:, 5, :] = -8.0                                                                 # a constant feature (a power of two): std 0
    total = sum(lens)
    o = Out((total, f), dtype, DEV)
    F.qn_normalize_pack(x, cu_of(lens), total, dtype, out=o.t)
    torch.cuda.synchronize()
    got = o.check("qn_normalize_pack").double()
    u, start = 2.0 ** -24, 0
    for b, n in enumerate(lens):
        xs = x[b, :, :n].double()
        m = xs.mean(1, keepdim=True)
        s = xs.std(1, unbiased=True, keepdim=True) + 1e-5
        v = ((xs - m) / s).t()                                                        # [n, F]
        big = xs.abs().max(1, keepdim=True).values
        dm = (n + 1) * u * big
        ds = dm + (n + 6) * u * s
        dv = ((2 * u * big + dm) / s).t() + v.abs() * (ds / s + 2 * u).t()
        bar = ulp16(v, dtype) / 2 + 2 * dv
        err = (got[start:start + n] - v).abs()
        print("normalize_pack %s len %d: max err / bar %.3f" % (dtype, n, float((err / bar).max())))
        assert bool((err <= bar).all()), "len %d: %d elements over the bar" % (n, int((err > bar).sum()))
        assert bool((got[start:start + n, 5] == 0).all()), "a constant feature must give 0 / 1e-5 = 0"
        start += n


def test_normalize_pack_argument_checks():
    x = torch.zeros((1, 64, 8), device=DEV)
    with pytest.raises(ValueError, match="16-bit output only"):
        F.qn_normalize_pack(x, cu_of([8]), 8, torch.float32)
    with pytest.raises(ValueError, match="F must be a multiple of 8"):
        F.qn_normalize_pack(torch.zeros((1, 60, 8), device=DEV), cu_of([8]), 8, BF)


# ---------------------------------------------------------------------------------------------------------------- ctc_greedy_packed
def _logits_for(rows, n_classes, ld, g):
    """rows: a list of class ids (or (id, id) for an exact tie between the two): the named class gets the largest logit."""
    x = torch.randn((len(rows), ld), generator=g, device=DEV)
    x[:, n_classes:] = 1e30                                                          # padding columns: must never win
    for r, c in enumerate(rows):
        if isinstance(c, tuple):
            x[r, c[0]] = x[r, c[1]] = 9.0
        else:
            x[r, c] = 9.0
    return x


def test_ctc_greedy_constructed_cases():
    nc, ld = 29, 32
    blank, a, b = nc - 1, 1, 2
    seqs = [
        [a, a, blank, a, b, b],            # "a a _ a b b" -> a a b
        [blank] * 5,                       # all blanks -> nothing
        [a],                               # length 1; and the NEXT sequence starts with the same id: must not merge
        [a, a, (3, 7), (blank, 4)],        # -> a, then tie 3 | 7 -> 3, then tie blank | 4 -> 4 (the first maximum)
        [],                                # length 0
        [b] * 300 + [blank, b],            # more than one block of 256 rows -> b b
    ]
    want_tokens = [[a, a, b], [], [a], [a, 3, 4], [], [b, b]]
    g = gen(DEV, 61)
    rows = [c for s in seqs for c in s]
    x = _logits_for(rows, nc, ld, g)
    lens = [len(s) for s in seqs]
    total = sum(lens)
    o_lp, o_id, o_tk = Out((total, nc), torch.float32, DEV), Out((total,), torch.int32, DEV), Out((total,), torch.int32, DEV)
    o_n = Out((len(seqs),), torch.int32, DEV)
    F.ctc_greedy_packed(x, cu_of(lens), nc, logp_out=o_lp.t, ids_out=o_id.t, tokens_out=o_tk.t, n_tokens_out=o_n.t)
    torch.cuda.synchronize()
    logp, ids, tokens, n_tok = o_lp.check("logp"), o_id.check("ids"), o_tk.check("tokens"), o_n.check("n_tokens")
    want_ids = [min(c) if isinstance(c, tuple) else c for c in rows]
    assert ids.tolist() == want_ids
    assert n_tok.tolist() == [len(t) for t in want_tokens]
    start = 0
    for n, t in zip(lens, want_tokens):
        assert tokens[start:start + len(t)].tolist() == t
        start += n
    ref = torch.log_softmax(x[:, :nc].double(), dim=1)
    bar = (nc + 8) * 2.0 ** -24 * (1 + ref.abs()) + 2.0 ** -22
    err = (logp.double() - ref).abs()
    print("ctc logp: max err / bar %.3f" % float((err / bar).max()))
    assert bool((err <= bar).all())
    # without logp: the same ids and tokens
    _, ids2, tok2, n2 = F.ctc_greedy_packed(x, cu_of(lens), nc, want_logp=False)
    torch.cuda.synchronize()
    assert torch.equal(ids2, ids) and torch.equal(n2, n_tok)
    start = 0
    for n, t in zip(lens, want_tokens):
        assert tok2[start:start + len(t)].tolist() == t
        start += n
