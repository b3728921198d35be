"""dle_conv1d_bn_packed_fwd (csrc/jasper.hip) and dle_qn_normalize_pack_lead (csrc/quartznet.hip) against float64, per element,
nothing skipped.  GPU only.

dle_conv1d_bn_packed_fwd -- contract (include/dle_mi355x.h), per output row p of sequence b:
    acc     = sum_k sum_c w[ko,k,c] x[cu_in[b] + p stride + (k - ksize/2) dilation, c]                     (0 outside the sequence)
    y[p,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) + residual[p,ko] ) )
Reference: torch float64 on the GPU, per sequence over a zero-padded copy, one strided slice per tap (no conv1d, nothing of this
library).

Bit-exact cases (tests/_exact_grid.py).  x, w, residual = k / 4 with |k| <= 4: every product is a multiple of 1/16 of magnitude <=
1 and the magnitude sum of an output's terms is at most ksize C <= 29 * 768 = 22,272 < B_MFMA, so the fp32 accumulator is exact in
any order (check_exact on the terms of the output with the largest magnitude sum; the sum is asserted below B_MFMA for all).  scale
is one of +-0.5, +-1, +-2 and shift a multiple of 1/16: the value before the rounding is a multiple of 1/32 below 2^16 (asserted),
exact in fp32, and y is the float64 value rounded ONCE.

Random cases against a derived, not measured, bar:
    |y - y64| <= ulp16(y64) / 2 + (ksize C + 3) 2^-24 (|scale| sum |w x| + |shift| + |residual|)
(one rounding + a (ksize C)-term fp32 sum, one fmaf, one addition).

Tile sizes the cases are named after: the kernel takes tiles of T = 128 OUTPUT rows per sequence, 128 output channels per
workgroup (a wavefront owns 64 rows x 64 channels), C in chunks of 64.  The kernel is not persistent, and its loop has one form.
  conv1_s2   64 -> 256, k 11, stride 2, lens 37, 6, 1        odd and even lengths, a sequence shorter than the half-kernel
  b1         256 -> 256, k 11, lens 127, 128, 129, 257       T - 1, T, T + 1, 2 T + 1: the row-tile edges
  b2_widen   256 -> 384, k 13, lens 80, 3                    three channel blocks
  b3         512 -> 512, k 17, lens 70
  b4         640 -> 640, k 21, lens 70                       ten chunks
  b5         768 -> 768, k 25, lens 70, 1
  conv2_d2   768 -> 896, k 29, dilation 2, lens 100, 44, 1   a halo of 28 rows longer than a sequence
  conv3      896 -> 1024, k 1, lens 5
  many_tiles 64 -> 64, k 3, 300 sequences of 129 rows        600 workgroups, more than the device has CUs; 300 sequences take five
                                                             steps of the 64-sequence tile search; Ko = 64: half a channel block
each in bf16 and fp16, with residual + ReLU, with neither, and with ReLU only (the ReLU cases assert that something was clipped).

Also: each sequence of b1 and conv2_d2 run alone equals, bit for bit, its rows when packed between neighbours filled with +-1e4; a
zero-length sequence in the middle of a batch; an inf in the last input row of a sequence reaches the rows whose window holds it
and no other (the zero rows beyond the sequence and the next sequence stay finite); argument checks raise without a launch, each
matched on its message.

dle_qn_normalize_pack_lead -- F = 64, lens (2, 3, 161), lead 16: the lead rows are exactly zero, the other rows equal, bit for bit,
dle_qn_normalize_pack on the same input, and lead 0 gives the bits of the old entry point.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests._exact_grid import B_MFMA, Out, assert_same, bits, check_exact, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
F64 = torch.float64
DEV = "cuda"
T = 128

# name -> (C, Ko, ksize, stride, dilation, lens)
SHAPES = {
    "conv1_s2": (64, 256, 11, 2, 1, (37, 6, 1)),
    "b1": (256, 256, 11, 1, 1, (T - 1, T, T + 1, 2 * T + 1)),
    "b2_widen": (256, 384, 13, 1, 1, (80, 3)),
    "b3": (512, 512, 17, 1, 1, (70,)),
    "b4": (640, 640, 21, 1, 1, (70,)),
    "b5": (768, 768, 25, 1, 1, (70, 1)),
    "conv2_d2": (768, 896, 29, 1, 2, (100, 44, 1)),
    "conv3": (896, 1024, 1, 1, 1, (5,)),
    "many_tiles": (64, 64, 3, 1, 1, (T + 1,) * 300),
}
MODES = {"res_relu": (True, True), "plain": (False, False), "relu": (False, True)}


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32, device=DEV)


def out_lens(lens, stride):
    return [(n - 1) // stride + 1 if n > 0 else 0 for n in lens]


def ref_conv(x, w, lens, stride, dilation):
    """(acc64, mag) [total_out, Ko] float64: per sequence over a zero-padded copy, one strided slice per tap.  w [Ko, ksize, C]."""
    x, w = x.to(F64), w.to(F64)
    ks = w.shape[1]
    halo = (ks // 2) * dilation
    accs, mags, start = [], [], 0
    for n in lens:
        seq = x[start:start + n]
        start += n
        if n == 0:
            continue
        ol = (n - 1) // stride + 1
        xp = torch.nn.functional.pad(seq, (0, 0, halo, halo))
        a = torch.zeros((ol, w.shape[0]), dtype=F64, device=x.device)
        m = torch.zeros_like(a)
        for k in range(ks):
            rows = xp[k * dilation:k * dilation + stride * (ol - 1) + 1:stride]
            a += rows @ w[:, k, :].t()
            m += rows.abs() @ w[:, k, :].abs().t()
        accs.append(a)
        mags.append(m)
    return torch.cat(accs), torch.cat(mags)


def run(x, w, scale, shift, lens, stride, dilation, residual, relu):
    ol = out_lens(lens, stride)
    total_out = sum(ol)
    cu_in = cu_of(lens)
    cu_out = cu_of(ol) if stride != 1 else None
    oy = Out((total_out, w.shape[0]), x.dtype, DEV)
    y = F.conv1d_bn_packed_fwd(x, w, scale, shift, cu_in, cu_out, total_out if stride != 1 else None, stride=stride,
                               dilation=dilation, residual=residual, relu=relu, out=oy.t)
    assert y.data_ptr() == oy.t.data_ptr()
    torch.cuda.synchronize()
    return oy.check("conv1d_bn_packed_fwd y")


def signs(n, g):
    return (torch.randint(0, 2, (n,), generator=g, device=DEV) * 2 - 1).float()


@functools.lru_cache(maxsize=None)
def exact_case(name, dtype):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    total = sum(lens)
    x = grid((total, c), 11, dtype, DEV)
    w = grid((ko, ks, c), 12, dtype, DEV)
    g = gen(DEV, 13)
    scale = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (ko,), generator=g, device=DEV)] * signs(ko, g)
    shift = torch.randint(-64, 65, (ko,), generator=g, device=DEV).float() / 16
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    acc, mag = ref_conv(x, w, lens, stride, dil)
    assert float(mag.max()) <= ks * c and float(mag.max()) < B_MFMA
    # the terms of the output with the largest magnitude sum, as a [ksize C, 1] column: on the 1/16 grid, summable exactly
    flat = int(mag.argmax())
    row, col = flat // ko, flat % ko
    ol, starts_in, starts_out, b = out_lens(lens, stride), [0], [0], 0
    for n, o in zip(lens, ol):
        starts_in.append(starts_in[-1] + n)
        starts_out.append(starts_out[-1] + o)
    while row >= starts_out[b + 1]:
        b += 1
    p = row - starts_out[b]
    terms = []
    for k in range(ks):
        t = p * stride + (k - ks // 2) * dil
        if 0 <= t < lens[b]:
            terms.append(x[starts_in[b] + t].double() * w[col, k].double())
    terms = torch.cat(terms).reshape(-1, 1)
    check_exact(terms, bound=B_MFMA)
    assert float(terms.abs().sum()) == float(mag.max()) and float(terms.sum()) == float(acc[row, col])
    res = grid((acc.shape[0], ko), 15, dtype, DEV)
    return x, w, scale, shift, res, acc


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv1d_bn_exact_grid_bits(name, dtype, mode):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    use_res, relu = MODES[mode]
    x, w, scale, shift, res, acc = exact_case(name, dtype)
    pre = scale.double() * acc + shift.double()
    if use_res:
        pre = pre + res.double()
    assert torch.equal(pre * 32, torch.round(pre * 32)) and float(pre.abs().max()) < 2.0 ** 16
    want = pre
    if relu:
        assert bool((pre < 0).any()), "nothing for the ReLU to clip"
        want = pre.clamp_min(0)
    y = run(x, w, scale, shift, lens, stride, dil, res if use_res else None, relu)
    assert_same(bits(y), bits(want.float().to(dtype)), "%s %s %s y" % (name, dtype, mode))


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    total = sum(lens)
    g = gen(DEV, 21)
    x = torch.randn((total, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, ks, c), generator=g, device=DEV) * (ks * c) ** -0.5).to(dtype)
    scale = (torch.rand((ko,), generator=g, device=DEV) * 3.75 + 0.25) * signs(ko, g)
    shift = torch.randn((ko,), generator=g, device=DEV)
    res = torch.randn((sum(out_lens(lens, stride)), ko), generator=g, device=DEV).to(dtype)
    acc, mag = ref_conv(x, w, lens, stride, dil)
    return x, w, scale, shift, res, acc, mag


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv1d_bn_random_inputs_derived_bar(name, dtype, mode):
    c, ko, ks, stride, dil, lens = SHAPES[name]
    use_res, relu = MODES[mode]
    x, w, scale, shift, res, acc, mag = random_case(name, dtype)
    y = run(x, w, scale, shift, lens, stride, dil, res if use_res else None, relu)
    ref = scale.double() * acc + shift.double()
    rmag = torch.zeros_like(ref)
    if use_res:
        ref = ref + res.double()
        rmag = res.double().abs()
    if relu:
        assert bool((ref < 0).any()), "nothing for the ReLU to clip"
        ref = ref.clamp_min(0)
    bar = ulp16(ref, dtype) / 2 + (ks * c + 3) * 2.0 ** -24 * (scale.double().abs() * mag + shift.double().abs() + rmag)
    err = (y.double() - ref).abs()
    worst = float((err / bar).max())
    print("%s %s %s: max err / bar %.3f" % (name, dtype, mode, worst))
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bar).all()), "%s y: %d of %d over the bar, worst ratio %.3f" % (name, int((err > bar).sum()), err.numel(), worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["b1", "conv2_d2"])
def test_conv1d_bn_sequences_are_isolated(name, dtype):
    """Sequence i alone == its rows when every OTHER sequence of the batch holds +-1e4 (and the residual rows of the others too)."""
    c, ko, ks, stride, dil, lens = SHAPES[name]
    x, w, scale, shift, res, _, _ = random_case(name, dtype)
    g = gen(DEV, 31)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    for i, n in enumerate(lens):
        lo, hi = starts[i], starts[i + 1]
        loud = (signs(x.numel(), g).view_as(x) * 1e4).to(dtype)
        loud[lo:hi] = x[lo:hi]
        y_all = run(loud, w, scale, shift, lens, stride, dil, res, True)
        y_one = run(x[lo:hi].contiguous(), w, scale, shift, [n], stride, dil, res[lo:hi].contiguous(), True)
        assert_same(bits(y_all[lo:hi]), bits(y_one), "%s sequence %d y" % (name, i))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv1d_bn_zero_length_sequence_mid_batch(dtype):
    c, ko, ks = 64, 64, 5
    g = gen(DEV, 41)
    lens_a, lens_b = [9, 0, 140, 0], [9, 140]
    x = torch.randn((149, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, ks, c), generator=g, device=DEV) * 0.1).to(dtype)
    scale, shift = torch.ones(ko, device=DEV), torch.zeros(ko, device=DEV)
    for stride in (1, 2):
        ya = run(x, w, scale, shift, lens_a, stride, 1, None, False)
        yb = run(x, w, scale, shift, lens_b, stride, 1, None, False)
        assert_same(bits(ya), bits(yb), "zero-length y stride %d" % stride)
        assert bool(torch.isfinite(ya).all())
    # a batch of nothing but empty sequences launches nothing and returns an empty output
    e = F.conv1d_bn_packed_fwd(x[:0], w, scale, shift, cu_of([0, 0]))
    assert tuple(e.shape) == (0, ko)


def test_conv1d_bn_an_inf_row_stays_inside_its_windows():
    """Positive weights, ksize 5, dilation 2: an inf in the LAST input row t of sequence 0 belongs to output rows t - 4, t - 2 and t
    of that sequence only.  The rows beyond the sequence are staged as zeros and never multiplied into another row's sum, and the
    next sequence does not see it."""
    c, n = 64, 50
    g = gen(DEV, 71)
    x = torch.randn((2 * n, c), generator=g, device=DEV).to(HF)
    x[n - 1, :] = float("inf")
    w = (torch.rand((c, 5, c), generator=g, device=DEV) + 0.5).to(HF)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y = run(x, w, sc, sh, [n, n], 1, 2, None, False)
    hit = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
    hit[[n - 5, n - 3, n - 1]] = True
    assert bool(torch.isinf(y[hit]).all())
    assert bool(torch.isfinite(y[~hit]).all())


def test_conv1d_bn_argument_checks_raise_without_a_launch():
    c = 64
    x = torch.zeros((8, c), dtype=BF, device=DEV)
    w = torch.zeros((c, 3, c), dtype=BF, device=DEV)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    cu = cu_of([8])
    F.conv1d_bn_packed_fwd(x, w, sc, sh, cu)                                     # the baseline call is inside the envelope
    with pytest.raises(ValueError, match=r"ksize must be odd in \[1, 29\] \(got 31\)"):
        F.conv1d_bn_packed_fwd(x, torch.zeros((c, 31, c), dtype=BF, device=DEV), sc, sh, cu)
    with pytest.raises(ValueError, match=r"ksize must be odd in \[1, 29\] \(got 4\)"):
        F.conv1d_bn_packed_fwd(x, torch.zeros((c, 4, c), dtype=BF, device=DEV), sc, sh, cu)
    with pytest.raises(ValueError, match="not both 2"):                         # stride 2 with dilation 2
        F.conv1d_bn_packed_fwd(x, w, sc, sh, cu, cu_of([4]), 4, stride=2, dilation=2)
    with pytest.raises(ValueError, match=r"C must be a multiple of 64 in \[64, 1024\] \(got 72\)"):
        F.conv1d_bn_packed_fwd(torch.zeros((8, 72), dtype=BF, device=DEV), torch.zeros((c, 3, 72), dtype=BF, device=DEV), sc, sh, cu)
    with pytest.raises(ValueError, match="16-bit activations and weights only"):  # fp32
        F.conv1d_bn_packed_fwd(x.float(), w.float(), sc, sh, cu)
    mis = torch.ones(c + 1, device=DEV)[1:]                                     # a misaligned operand
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    with pytest.raises(ValueError, match="16-byte aligned"):
        F.conv1d_bn_packed_fwd(x, w, mis, sh, cu)
    with pytest.raises(ValueError, match="y must not overlap"):                 # y aliasing x
        F.conv1d_bn_packed_fwd(x, w, sc, sh, cu, out=x)
    y = torch.zeros((8, c), dtype=BF, device=DEV)
    args = [C.ptr(x), C.ptr(w), C.ptr(sc), C.ptr(sh), 0, C.ptr(y), C.ptr(cu), C.ptr(cu)]
    tail = (1, 8, 8, c, c, 3, 1, 1, 1, C.dt(BF), C.stream())
    for i in (0, 1, 2, 3, 5, 6, 7):                                             # every pointer but residual, which may be null
        bad = list(args)
        bad[i] = 0
        with pytest.raises(ValueError, match="null pointer"):
            C.call("dle_conv1d_bn_packed_fwd", *bad, *tail)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- normalize_pack_lead
@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_pack_lead_rows_and_bits(dtype):
    f, t_pad, lens, lead = 64, 168, (2, 3, 161), 16
    g = gen(DEV, 51)
    x = torch.randn((len(lens), f, t_pad), generator=g, device=DEV) * 3 - 7
    total = sum(lens)
    old = Out((total, f), dtype, DEV)
    F.qn_normalize_pack(x, cu_of(lens), total, dtype, out=old.t)
    padded = [n + lead for n in lens]
    new = Out((sum(padded), f), dtype, DEV)
    F.qn_normalize_pack_lead(x, cu_of(padded), sum(padded), dtype, lead, out=new.t)
    zero = Out((total, f), dtype, DEV)
    F.qn_normalize_pack_lead(x, cu_of(lens), total, dtype, 0, out=zero.t)
    torch.cuda.synchronize()
    want, got, got0 = old.check("qn_normalize_pack"), new.check("qn_normalize_pack_lead"), zero.check("qn_normalize_pack_lead 0")
    assert bool(torch.isfinite(want).all())
    assert_same(bits(got0), bits(want), "lead 0 against the old entry point")
    a = b = 0
    for n in lens:
        assert_same(bits(got[b:b + lead]), torch.zeros((lead, f), dtype=torch.int16, device=DEV), "the lead rows")
        assert_same(bits(got[b + lead:b + lead + n]), bits(want[a:a + n]), "the rows behind the lead")
        a, b = a + n, b + lead + n
    with pytest.raises(ValueError, match="lead must be"):
        F.qn_normalize_pack_lead(x, cu_of(lens), total, dtype, -1)
