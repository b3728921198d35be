"""dle_conv2d_grouped_fwd_affine -- the grouped 3x3 / pad 1 convolution of the ResNeXt bottleneck with the evaluation-mode BatchNorm
and the ReLU in its epilogue -- against float64.  GPU only.

Contract:  y[n,p,q,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) ) ),  acc the fp32 accumulator over the 16-bit weights of
ko's group only; x [N,H,W,C], w [Ko,3,3,Cg] (torch's grouped OIHW weight permuted (0,2,3,1)).

Reference.  torch float64 on the GPU: per group and per tap a matrix product over a padded, strided slice (no conv2d, nothing of
this library), then scale * acc + shift, ReLU.

Bit-exact cases.  x, w = k / 4 with |k| <= 4 (tests/_exact_grid.py): every product is a multiple of 1/16 of magnitude at most 1, a
contraction has at most 9 * 32 = 288 terms -- far below B_MFMA -- so the fp32 accumulator is exact in any order.  scale is one of
+-0.5, +-1, +-2 (both signs present) and shift a multiple of 1/16: the value before the rounding is a multiple of 1/32 below 2^19,
exact in fp32, and the output is the float64 value rounded ONCE.  Both preconditions are asserted on the float64 side.  ReLU on and
off; the ReLU cases assert that something was clipped.

Random inputs.  x ~ N(0,1), w ~ N(0, 1/(9 Cg)), |scale| in [0.25, 4] with random signs, shift ~ N(0,1), all rounded to storage
first.  Per element, nothing skipped:
    |got - ref| <= ulp16(ref) / 2 + (9 Cg + 2) 2^-24 (|scale| sum|x w| + |shift|)
half a unit of the 16-bit format at the reference value (the one rounding) plus the fp32 error of a 9 Cg-term sum and one fmaf.
The bar is derived, not measured.  (The kernel also adds exact zero products for the other groups of a 32-channel block: they
contribute no rounding.)

Shapes (N,H,W,C,Cg,stride) -- the smallest at which each feature can fail.  The kernel (csrc/conv_grouped.hip) walks 32-pixel
tiles of the FLAT output index (n,p,q) per 32-channel block, `walkers` wavefronts per block (at most 8 x CUs / blocks):
* s1_128_g4 (2,14,14,128,4,1), s1_256_g8 (1,12,20,256,8,1; non-square), s2_256_g8 (2,14,14,256,8,2), s1_512_g16 (3,9,11,512,16,1),
  s2_512_g16_odd (1,15,15,512,16,2: an odd extent with stride 2), s1_1024_g32 (1,7,7,1024,32,1), s2_1024_g32 (2,14,14,1024,32,2):
  every Cg with both strides as the network runs them; 392 = 12.25 tiles: a ragged last tile, tiles that span the two images;
* pad_2x2 (1,2,2,1024,32,1): padding dominates (a 64 x 64 image reaches this); one tile with 4 live pixels;
* four_groups (1,8,8,64,16,1): 4 groups, catches a hard-coded 32; two channel blocks only (half a workgroup);
* span3_ragged (3,5,7,128,4,2): 12 output pixels per image: the first tile spans all three images, the last holds 4 pixels;
* multi_trip (6,56,56,128,4,1): 588 tiles for at most 512 walkers per block on a 256-CU device: some wavefronts take a second tile
  with the weights they kept in registers.

Argument checks (no launch): Cg = 2, stride 3, C != Ko, fp32, a misaligned operand raise ValueError.

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

# name -> (N, H, W, C, Cg, stride)
SHAPES = {
    "s1_128_g4": (2, 14, 14, 128, 4, 1),
    "s1_256_g8": (1, 12, 20, 256, 8, 1),
    "s2_256_g8": (2, 14, 14, 256, 8, 2),
    "s1_512_g16": (3, 9, 11, 512, 16, 1),
    "s2_512_g16_odd": (1, 15, 15, 512, 16, 2),
    "s1_1024_g32": (1, 7, 7, 1024, 32, 1),
    "s2_1024_g32": (2, 14, 14, 1024, 32, 2),
    "pad_2x2": (1, 2, 2, 1024, 32, 1),
    "four_groups": (1, 8, 8, 64, 16, 1),
    "span3_ragged": (3, 5, 7, 128, 4, 2),
    "multi_trip": (6, 56, 56, 128, 4, 1),
}


def ref_grouped(x, w, stride):
    """(acc, mag) [N, P, Q, Ko] float64: the grouped convolution of x [N,H,W,C] with w [Ko,3,3,Cg] and the sum of |x w| per output,
    as per-group, per-tap matrix products over padded strided slices."""
    x, w = x.to(F64), w.to(F64)
    n, h, wd, c = x.shape
    ko, _, _, cg = w.shape
    groups = c // cg
    kg = ko // groups
    p, q = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros((n * p * q, groups, kg), dtype=F64, device=x.device)
    mag = torch.zeros_like(acc)
    for i in range(3):
        for j in range(3):
            win = xp[:, i:i + stride * (p - 1) + 1:stride, j:j + stride * (q - 1) + 1:stride, :].reshape(n * p * q, groups, cg)
            wt = w[:, i, j, :].reshape(groups, kg, cg)
            # per group g: [M, cg] @ [cg, kg]
            acc += torch.bmm(win.transpose(0, 1), wt.transpose(1, 2)).transpose(0, 1)
            mag += torch.bmm(win.abs().transpose(0, 1), wt.abs().transpose(1, 2)).transpose(0, 1)
    return acc.reshape(n, p, q, ko), mag.reshape(n, p, q, ko)


def run(x, w, scale, shift, groups, stride, relu):
    n, h, wd, c = x.shape
    p, q = (h - 1) // stride + 1, (wd - 1) // stride + 1
    o = Out((n, p, q, w.shape[0]), x.dtype, DEV)
    y = F.conv2d_grouped_fwd_affine(x, w, scale, shift, groups, stride, relu=relu, out=o.t)
    assert y.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    return o.check("conv2d_grouped_fwd_affine")


@functools.lru_cache(maxsize=None)
def exact_case(name, dtype):
    n, h, wd, c, cg, stride = SHAPES[name]
    x = grid((n, h, wd, c), 11, dtype, DEV)
    w = grid((c, 3, 3, cg), 12, dtype, DEV)
    g = gen(DEV, 13)
    scale = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (c,), generator=g, device=DEV)]
    scale = scale * (torch.randint(0, 2, (c,), generator=g, device=DEV) * 2 - 1).float()
    shift = torch.randint(-64, 65, (c,), generator=g, device=DEV).float() / 16
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    acc, mag = ref_grouped(x, w, stride)
    assert float(mag.max()) <= 288 < B_MFMA                              # at most 288 terms of at most 1 each
    assert torch.equal(acc * 16, torch.round(acc * 16))
    pre = scale.double() * acc + shift.double()
    assert torch.equal(pre * 32, torch.round(pre * 32)) and float(pre.abs().max()) < 2.0 ** 19
    return x, w, scale, shift, pre


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_grid_bits(name, dtype, relu):
    n, h, wd, c, cg, stride = SHAPES[name]
    x, w, scale, shift, pre = exact_case(name, dtype)
    want = pre
    if relu:
        assert bool((pre < 0).any()), "nothing for the ReLU to clip"
        want = pre.clamp_min(0)
    got = run(x, w, scale, shift, c // cg, stride, relu)
    assert_same(bits(got), bits(want.float().to(dtype)), "%s %s relu=%d" % (name, dtype, relu))


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    n, h, wd, c, cg, stride = SHAPES[name]
    g = gen(DEV, 21)
    x = torch.randn((n, h, wd, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((c, 3, 3, cg), generator=g, device=DEV) * (9 * cg) ** -0.5).to(dtype)
    scale = (torch.rand((c,), generator=g, device=DEV) * 3.75 + 0.25) * (torch.randint(0, 2, (c,), generator=g, device=DEV) * 2 - 1).float()
    shift = torch.randn((c,), generator=g, device=DEV)
    acc, mag = ref_grouped(x, w, stride)
    return x, w, scale, shift, acc, mag


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_inputs_per_element_bar(name, dtype, relu):
    n, h, wd, c, cg, stride = SHAPES[name]
    x, w, scale, shift, acc, mag = random_case(name, dtype)
    ref = scale.double() * acc + shift.double()
    if relu:
        ref = ref.clamp_min(0)
    got = run(x, w, scale, shift, c // cg, stride, relu).double()
    bar = ulp16(ref, dtype) / 2 + (9 * cg + 2) * 2.0 ** -24 * (scale.double().abs() * mag + shift.double().abs())
    err = (got - ref).abs()
    worst = float((err / bar).max())
    print("%s %s relu=%d: max err / bar %.3f" % (name, dtype, relu, worst))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bar).all()), "%s: %d of %d elements over the bar, worst ratio %.3f" % (name, int((err > bar).sum()), err.numel(), worst)


def test_argument_checks_raise_without_a_launch():
    c = 128
    x = torch.zeros((1, 4, 4, c), dtype=BF, device=DEV)
    w = torch.zeros((c, 3, 3, 4), dtype=BF, device=DEV)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    F.conv2d_grouped_fwd_affine(x, w, sc, sh, 32)                       # the baseline call is inside the envelope
    with pytest.raises(ValueError):                                     # Cg = 2
        F.conv2d_grouped_fwd_affine(x, torch.zeros((c, 3, 3, 2), dtype=BF, device=DEV), sc, sh, 64)
    with pytest.raises(ValueError):                                     # stride 3
        F.conv2d_grouped_fwd_affine(x, w, sc, sh, 32, stride=3)
    with pytest.raises(ValueError):                                     # C != Ko
        F.conv2d_grouped_fwd_affine(x, torch.zeros((2 * c, 3, 3, 4), dtype=BF, device=DEV), torch.ones(2 * c, device=DEV),
                                    torch.zeros(2 * c, device=DEV), 32)
    with pytest.raises(ValueError):                                     # fp32
        F.conv2d_grouped_fwd_affine(x.float(), w.float(), sc, sh, 32)
    # a misaligned operand: scale 4 bytes into a 16-byte aligned buffer
    mis = torch.ones(c + 1, device=DEV)[1:]
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    with pytest.raises(ValueError):
        F.conv2d_grouped_fwd_affine(x, w, mis, sh, 32)
    torch.cuda.synchronize()
