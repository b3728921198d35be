"""dle_conv1d_lrelu_fwd -- the dilated "same" Conv1d of the HiFi-GAN generator with the leaky ReLU in front of it and bias, two
addends and a scale in its epilogue -- and dle_hfg_post_fwd -- the one-channel output convolution with its tanh -- against
float64.  GPU only.

Contract:  a = x < 0 ? round16(fl32(float(x) * slope)) : x  (slope == 1: a = x);  acc = sum_k sum_c w[ko,k,c] a[b, t + (k -
(ksize-1)/2) dilation, c] on the fp32 accumulator, zero outside [0, T);  y = round16((acc + bias (+ add1) (+ add2)) * alpha);
x [B,T,C], w [Ko,ksize,C] (torch's Conv1d weight permuted (0,2,1)).  audio = tanhf(bias + sum_k sum_c w[k,c] a[b, t + k - (ksize-1)/2, c]).

Reference.  torch float64 on the GPU: per tap a matrix product over a zero-padded, shifted slice (no conv1d, nothing of this
library); `a` is (x.float() * slope).to(dtype) where x < 0 -- the contract, torch's own rounding.

Bit-exact cases.  x, w, add1, add2 = k / 4 with |k| <= 4 (tests/_exact_grid.py), slope in {1, 0.25}, alpha in {1, 0.5}, bias a
multiple of 1/64: `a` is a multiple of 1/16 (exact in both types), every term a multiple of 1/64 of magnitude at most 1, at most
11 * 512 = 5,632 of them -- the sum of magnitudes, addends and bias included, stays below B_MFMA = 2^18, so every partial sum in any
order has at most 24 significant bits and the fp32 accumulator is exact; times alpha it is a multiple of 1/128 below 2^17, still
exact; the output is the float64 value rounded ONCE.  The preconditions are asserted on the float64 side.  Variants: no addend;
add1; add1 + add2; add1 + add2 with the output written over add2 (the header allows y to BE an addend).  The lrelu variants assert
that negative inputs occurred.

Random inputs with the network's constants: slope 0.1, alpha = fp32(1/3), both addends; x, add ~ N(0,1), w ~ N(0, 1/(ksize C)),
bias ~ N(0,1), all rounded to storage first.  Per element, nothing skipped:
    |got - ref| <= ulp16(ref) / 2 + (ksize C + 5) 2^-24 |alpha| (sum|w a| + |bias| + |add1| + |add2|)
half a unit of the 16-bit format at the reference value (the one rounding) plus the fp32 error of a (ksize C)-term sum, three
additions, one product.  The bar is derived, not measured.

Shapes (B,T,C,Ko,ksize,dilation) -- the smallest at which each feature can fail.  The kernel (csrc/hifigan.hip) gives a workgroup
of 4 wavefronts TT time steps of ONE image x 32 WK output channels, (WK, TT) = (1, 256) for Ko <= 32, (2, 128) for Ko <= 64,
(4, 64) above; a wavefront owns two 32-step sub-tiles; C is staged in chunks of 64 channels, 16 per MFMA:
* pre_c80 (2,37,80,64,7,1): conv_pre's C = 80 = one whole chunk + a 16-channel one; WK = 2, one ragged tile per image;
* short_t (1,5,32,32,11,5): T = 5 shorter than the 25-step halo: every tap but the centre one reads padding on one side at least;
* one (1,1,8,8,3,1): one step, half a 16-channel MFMA step (zero filled), 8 of a wavefront's 32 channels live;
* tiles300 (3,300,64,64,3,3): WK = 2, TT = 128: three time tiles per image, the last with 44 steps; the tile boundaries at 128 and
  256 lie inside the 3-step halo of both neighbours; image b's first and last 3 steps hold +-1 of a sign that alternates with b, so
  a tap that read across an image boundary instead of padding would change the sums of every channel;
* wide (2,130,256,256,11,5): WK = 4, TT = 64: three tiles, the last with 2 steps (one live sub-tile row); 4 chunks of C; 2 channel blocks;
* up_2048 (1,9,512,2048,3,1): the packed stage-1 upsample: 16 channel blocks, 8 chunks;
* narrow (2,70,16,8,7,1), halo24 (1,40,8,8,5,12) and halo36 (1,40,8,8,7,12: the widest halo): the narrow ends of the envelope;
  T = 40 shorter than two halos;
* blocks_40 (1,33,24,40,3,2): Ko = 40: WK = 2, the second wavefront's block has 8 live channels; C = 24: one and a half MFMA steps;
* stage4_600 (2,600,32,32,7,3): the WK = 1, TT = 256 instantiation that carries the network's last stage: three time tiles per
  image, the boundaries at 256 and 512 inside the 9-step halo of both neighbours, a ragged last tile of 88 steps (its wavefronts own
  64, 24, 0 and 0 of them: a partly filled sub-tile and two idle wavefronts that still stage and meet the barriers).
The kernel is not persistent (one workgroup per tile), so no multi-pass shape exists.

Upsample end to end: functional.pack_upsample_weight + the kernel against float64 conv_transpose1d under the same bar (3 Cin
terms), (u, k, Cin, Cout) = (8, 16, 64, 32) and (2, 4, 16, 8) at T = 7.

Post kernel, the same two tiers, shapes (B,T,C,ksize) = (2,50,32,7), (1,3,8,7), (3,700,64,11) (three 256-step tiles, ragged).
Grid inputs (w = +-1/4 at 30 % density so that the arguments stay where tanh is not saturated -- asserted): the argument is exact
in fp32 and  |got - tanh64(arg)| <= c 2^-24.  Random inputs:  |got - tanh64(arg)| <= (ksize C + 2) 2^-24 sum|terms| + c 2^-24
(tanh is 1-Lipschitz).  c is not derived: as tests/test_gpu_se_ops.py does for the sigmoid it is measured here, on the device, as
max |torch.tanh(z_fp32) - tanh64(z)| / 2^-24 over a dense grid of z in [-12, 12] -- torch's kernel, not the one under test -- and
the bar allows twice that value (two independent implementations may each be off by their own unit).  Measured: c = 1.38; the yardstick itself is asserted inside (0, 16).

Argument checks (no launch): C = 12, even ksize, halo 40, fp32, a misaligned operand, y aliasing x raise ValueError.

Outputs are views at the head of over-long NaN-filled buffers: the tail must keep its bits.
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
U = 2.0 ** -24

# name -> (B, T, C, Ko, ksize, dilation)
SHAPES = {
    "pre_c80": (2, 37, 80, 64, 7, 1),
    "short_t": (1, 5, 32, 32, 11, 5),
    "one": (1, 1, 8, 8, 3, 1),
    "tiles300": (3, 300, 64, 64, 3, 3),
    "wide": (2, 130, 256, 256, 11, 5),
    "up_2048": (1, 9, 512, 2048, 3, 1),
    "narrow": (2, 70, 16, 8, 7, 1),
    "halo24": (1, 40, 8, 8, 5, 12),
    "halo36": (1, 40, 8, 8, 7, 12),
    "blocks_40": (1, 33, 24, 40, 3, 2),
    "stage4_600": (2, 600, 32, 32, 7, 3),
}
# name -> (slope, alpha, addends, output written over add2)
VARIANTS = {
    "plain": (1.0, 1.0, 0, False),
    "lrelu_add1": (0.25, 1.0, 1, False),
    "lrelu_both_half": (0.25, 0.5, 2, False),
    "both_half_inplace": (1.0, 0.5, 2, True),
}


def lrelu16(x, slope):
    """The contract's `a`: an fp32 product rounded to x's type where x < 0."""
    return x if slope == 1.0 else torch.where(x < 0, (x.float() * slope).to(x.dtype), x)


def ref_conv(a, w, dilation):
    """(acc, mag) [B, T, Ko] float64: sum over taps of a zero-padded shifted slice of a [B,T,C] times w[:, k, :]^T, and the sum of
    |w a| per output."""
    a, w = a.to(F64), w.to(F64)
    b, t, c = a.shape
    ko, ks, _ = w.shape
    halo = (ks - 1) // 2 * dilation
    ap = torch.nn.functional.pad(a, (0, 0, halo, halo))
    acc = torch.zeros((b, t, ko), dtype=F64, device=a.device)
    mag = torch.zeros_like(acc)
    for k in range(ks):
        win = ap[:, k * dilation:k * dilation + t, :]
        acc += win @ w[:, k, :].t()
        mag += win.abs() @ w[:, k, :].abs().t()
    return acc, mag


def run(x, w, bias, dilation, slope, alpha, add1, add2, inplace=False):
    b, t, _ = x.shape
    o = Out((b, t, w.shape[0]), x.dtype, DEV, fill=add2 if inplace else None)
    y = F.conv1d_lrelu_fwd(x, w, bias, dilation=dilation, slope=slope, alpha=alpha, add1=add1, add2=o.t if inplace else add2, out=o.t)
    assert y.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    return o.check("conv1d_lrelu_fwd")


@functools.lru_cache(maxsize=None)
def exact_inputs(name, dtype):
    b, t, c, ko, ks, dil = SHAPES[name]
    x = grid((b, t, c), 11, dtype, DEV)
    if name == "tiles300":                                               # image edges: +-1, the sign alternating with the image
        h = (ks - 1) // 2 * dil
        for i in range(b):
            x[i, :h] = 1.0 if i % 2 == 0 else -1.0
            x[i, t - h:] = -1.0 if i % 2 == 0 else 1.0
        assert bool((x[:, :h] != 0).all()) and bool((x[:, t - h:] != 0).all())
    w = grid((ko, ks, c), 12, dtype, DEV)
    bias = torch.randint(-64, 65, (ko,), generator=gen(DEV, 13), device=DEV).float() / 64
    add1, add2 = grid((b, t, ko), 14, dtype, DEV), grid((b, t, ko), 15, dtype, DEV)
    return x, w, bias, add1, add2


@functools.lru_cache(maxsize=None)
def exact_acc(name, dtype, slope):
    x, w, _, _, _ = exact_inputs(name, dtype)
    a = lrelu16(x, slope)
    assert torch.equal(a.double() * 16, torch.round(a.double() * 16))
    acc, mag = ref_conv(a, w, SHAPES[name][5])
    assert torch.equal(acc * 64, torch.round(acc * 64))
    assert float(mag.max()) + 3 < B_MFMA                                 # + |bias| + |add1| + |add2|, each at most 1
    return acc


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_grid_bits(name, dtype, variant):
    slope, alpha, n_add, inplace = VARIANTS[variant]
    x, w, bias, add1, add2 = exact_inputs(name, dtype)
    if slope != 1.0:
        assert bool((x < 0).any()), "no negative input for the leaky ReLU"
    pre = exact_acc(name, dtype, slope) + bias.double()
    if n_add >= 1:
        pre = pre + add1.double()
    if n_add >= 2:
        pre = pre + add2.double()
    pre = pre * alpha
    assert torch.equal(pre * 128, torch.round(pre * 128)) and float(pre.abs().max()) < 2.0 ** 17
    got = run(x, w, bias, SHAPES[name][5], slope, alpha, add1 if n_add >= 1 else None, add2 if n_add >= 2 else None, inplace)
    assert_same(bits(got), bits(pre.float().to(dtype)), "%s %s %s" % (name, dtype, variant))


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    b, t, c, ko, ks, dil = SHAPES[name]
    g = gen(DEV, 21)
    x = torch.randn((b, t, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, ks, c), generator=g, device=DEV) * (ks * c) ** -0.5).to(dtype)
    bias = torch.randn((ko,), generator=g, device=DEV)
    add1 = torch.randn((b, t, ko), generator=g, device=DEV).to(dtype)
    add2 = torch.randn((b, t, ko), generator=g, device=DEV).to(dtype)
    acc, mag = ref_conv(lrelu16(x, 0.1), w, dil)
    return x, w, bias, add1, add2, acc, mag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_inputs_per_element_bar(name, dtype):
    b, t, c, ko, ks, dil = SHAPES[name]
    x, w, bias, add1, add2, acc, mag = random_case(name, dtype)
    alpha = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))          # the fp32 value the kernel receives
    ref = (acc + bias.double() + add1.double() + add2.double()) * alpha
    got = run(x, w, bias, dil, 0.1, alpha, add1, add2).double()
    bar = ulp16(ref, dtype) / 2 + (ks * c + 5) * U * abs(alpha) * (mag + bias.double().abs() + add1.double().abs() + add2.double().abs())
    err = (got - ref).abs()
    worst = float((err / bar).max())
    print("%s %s: max err / bar %.3f" % (name, dtype, worst))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bar).all()), "%s: %d of %d elements over the bar, worst ratio %.3f" % (name, int((err > bar).sum()), err.numel(), worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(8, 16, 64, 32), (2, 4, 16, 8)], ids=["u8k16", "u2k4"])
def test_upsample_end_to_end_against_conv_transpose1d(case, dtype):
    u, k, cin, cout = case
    b, t = 2, 7
    g = gen(DEV, 31)
    x = torch.randn((b, t, cin), generator=g, device=DEV).to(dtype)
    w = (torch.randn((cin, cout, k), generator=g, device=DEV) * (cin * k / u) ** -0.5).to(dtype)
    bias = torch.randn((cout,), generator=g, device=DEV)
    packed = F.pack_upsample_weight(w, u, dtype)
    assert tuple(packed.shape) == (u * cout, 3, cin)
    a = lrelu16(x, 0.1).double().permute(0, 2, 1)
    ct = lambda inp, wt: torch.nn.functional.conv_transpose1d(inp, wt, None, u, (k - u) // 2).permute(0, 2, 1)
    ref = ct(a, w.double()) + bias.double()
    mag = ct(a.abs(), w.double().abs()) + bias.double().abs()
    assert tuple(ref.shape) == (b, t * u, cout)
    o = Out((b, t, u * cout), dtype, DEV)
    F.conv1d_lrelu_fwd(x, packed, bias.repeat(u), slope=0.1, out=o.t)
    torch.cuda.synchronize()
    got = o.check("conv1d_lrelu_fwd").view(b, t * u, cout).double()
    bar = ulp16(ref, dtype) / 2 + (3 * cin + 5) * U * mag
    err = (got - ref).abs()
    worst = float((err / bar).max())
    print("upsample %s %s: max err / bar %.3f" % (case, dtype, worst))
    assert bool((err <= bar).all()), "%d of %d elements over the bar, worst ratio %.3f" % (int((err > bar).sum()), err.numel(), worst)


# ---- the output kernel ---------------------------------------------------------------------------------------------------------
POST_SHAPES = [(2, 50, 32, 7), (1, 3, 8, 7), (3, 700, 64, 11)]


@functools.lru_cache(maxsize=None)
def tanh_units():
    """c: max |torch.tanh(z_fp32) - tanh64(z)| / 2^-24 over a dense grid of z in [-12, 12], on the device."""
    z = torch.linspace(-12.0, 12.0, 2000001, dtype=F64, device=DEV).float()
    z = torch.cat([z, torch.randn(1000000, generator=gen(DEV, 41), device=DEV)])
    err = (torch.tanh(z).double() - torch.tanh(z.double())).abs()
    c_u = float(err.max()) / U
    assert 0 < c_u < 16, "tanh yardstick %.3f u: torch's own tanh is off, the bars below would mean nothing" % c_u
    return c_u


def run_post(x, w, bias, slope):
    o = Out(tuple(x.shape[:2]), torch.float32, DEV)
    y = F.hfg_post_fwd(x, w, bias, slope=slope, out=o.t)
    assert y.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    return o.check("hfg_post_fwd")


@pytest.mark.parametrize("slope", [1.0, 0.25], ids=["linear", "lrelu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", POST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_post_exact_argument(shape, dtype, slope):
    b, t, c, ks = shape
    x = grid((b, t, c), 51, dtype, DEV)
    w = grid((ks, c), 52, dtype, DEV, kmax=1, density=0.3)
    bias = torch.tensor([5.0 / 64], device=DEV)
    assert slope == 1.0 or bool((x < 0).any())
    acc, mag = ref_conv(lrelu16(x, slope), w[None], 1)
    arg = acc[:, :, 0] + bias.double()
    assert torch.equal(arg * 64, torch.round(arg * 64)) and float(mag.max()) + 1 < 2.0 ** 18      # exact in fp32 in any order
    assert float((arg.abs() < 2).double().mean()) >= 0.5, "most arguments saturate the tanh"
    got = run_post(x, w, bias, slope)
    c_u = tanh_units()
    err = (got.double() - torch.tanh(arg)).abs()
    print("post exact %s %s slope %g: tanh yardstick c = %.3f u; max err %.3e = %.3f u" % (shape, dtype, slope, c_u, float(err.max()), float(err.max()) / U))
    assert bool((err <= 2 * c_u * U).all()), "max err %.3e against %.3e" % (float(err.max()), 2 * c_u * U)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", POST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_post_random_inputs_per_element_bar(shape, dtype):
    b, t, c, ks = shape
    g = gen(DEV, 61)
    x = torch.randn((b, t, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ks, c), generator=g, device=DEV) * (ks * c) ** -0.5).to(dtype)
    bias = torch.randn((1,), generator=g, device=DEV) * 0.1
    acc, mag = ref_conv(lrelu16(x, 0.01), w[None], 1)
    arg = acc[:, :, 0] + bias.double()
    got = run_post(x, w, bias, 0.01)
    c_u = tanh_units()
    bar = (ks * c + 2) * U * (mag[:, :, 0] + bias.double().abs()) + 2 * c_u * U
    err = (got.double() - torch.tanh(arg)).abs()
    worst = float((err / bar).max())
    print("post %s %s: max err / bar %.3f" % (shape, dtype, worst))
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    assert bool((err <= bar).all()), "%d of %d elements over the bar, worst ratio %.3f" % (int((err > bar).sum()), err.numel(), worst)


def test_argument_checks_raise_without_a_launch():
    z = lambda *s, dt=BF: torch.zeros(s, dtype=dt, device=DEV)
    x, w, bias = z(1, 16, 16), z(8, 3, 16), torch.zeros(8, device=DEV)
    F.conv1d_lrelu_fwd(x, w, bias)                                       # the baseline call is inside the envelope
    with pytest.raises(ValueError):                                      # C = 12
        F.conv1d_lrelu_fwd(z(1, 16, 12), z(8, 3, 12), bias)
    with pytest.raises(ValueError):                                      # even ksize
        F.conv1d_lrelu_fwd(x, z(8, 4, 16), bias)
    with pytest.raises(ValueError):                                      # halo 40
        F.conv1d_lrelu_fwd(x, z(8, 11, 16), bias, dilation=8)
    with pytest.raises(ValueError):                                      # fp32
        F.conv1d_lrelu_fwd(x.float(), w.float(), bias)
    mis = torch.zeros(9, device=DEV)[1:]                                 # a misaligned operand: bias 4 bytes into its buffer
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    with pytest.raises(ValueError):
        F.conv1d_lrelu_fwd(x, w, mis)
    sq = z(16, 3, 16)                                                    # C == Ko: y over x has the right shape
    with pytest.raises(ValueError):
        F.conv1d_lrelu_fwd(x, sq, torch.zeros(16, device=DEV), out=x)
    with pytest.raises(ValueError):                                      # the output kernel: C = 72, even ksize, fp32
        F.hfg_post_fwd(z(1, 16, 72), z(7, 72), torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):
        F.hfg_post_fwd(x, z(6, 16), torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):
        F.hfg_post_fwd(x.float(), z(7, 16).float(), torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
