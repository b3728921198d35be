"""dle_conv2d_fwd_affine -- the inference convolution with the evaluation-mode BatchNorm, the residual add and the ReLU in its
epilogue -- and the stem's affine + ReLU + max-pooling pass, against float64.  GPU only.

Contract:  y[n,p,q,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) + float(residual[n,p,q,ko]) ) ),  acc the fp32
accumulator of the convolution over the 16-bit operands.

Reference.  torch float64 on the GPU, the convolution written as a sum of per-tap matrix products over padded, strided slices (no
torch.nn.functional.conv2d, nothing of this library), then scale * acc + shift (+ residual), ReLU.

Bit-exact cases.  x, w and the residual are k / 4 with |k| <= 4 (tests/_exact_grid.py): every product is a multiple of 1/16, and
while the sum of magnitudes of a contraction stays below B_MFMA = 2^18 the fp32 accumulator is exact in any order.  scale is one of
+-0.5, +-1, +-2 and shift a multiple of 1/16, so scale * acc, + shift, + residual are multiples of 1/32; below 2^19 such a value has
at most 24 significant bits: the fmaf and the add are exact in fp32, and the output is the float64 value rounded ONCE to 16 bits
(float64 -> float32 exact here, torch's float32 -> 16-bit conversion is round-to-nearest-even).  Both preconditions are asserted
on the float64 side before anything is compared.  Each shape runs with the residual on / off and the ReLU on / off; the scale has
both signs, and the ReLU cases assert that something was clipped.

Shapes -- the smallest at which each route can still go wrong:
* halo-tile kernel (csrc/conv3x3.hip, AFF): (N,H,W,C,Ko) = (2,14,14,64,64): a 256-slot tile spans an image boundary, ragged last
  tile; (1,12,20,128,128): NT = 128, non-square, two channel chunks; (5,10,10,64,192): several images per tile, three N tiles.
  dle_conv3x3_affine_launch_count() must advance by one per call;
* 1x1 stride 1 as a plain matrix product on the tile kernel (csrc/gemm_dma.hip, PLAIN = 2), M x K x N = 98 x 64 x 256 (ragged M),
  392 x 256 x 64 (half a column tile), 49 x 2048 x 512 (long contraction: one image of the last stage);
* implicit GEMM: 1x1 stride 2 (2,14,14,256) -> 512; 3x3 stride 2 pad 1 (2,14,14,128) -> 128; 3x3 stride 1 at 7x7x512, which the
  halo kernel declines (its size rule): the counter must NOT move and the fallback must be exact.

Random inputs.  x ~ N(0,1), w ~ N(0,1/K), |scale| in [0.25, 4] with random signs, shift, residual ~ N(0,1), all rounded to their
storage types first; the reference runs on the rounded values.  Per element, nothing skipped:
    |got - ref| <= ulp16(ref) / 2 + (K + 3) 2^-24 (|scale| sum|x w| + |shift| + |residual|)
half a unit of the 16-bit format at the reference value (the one rounding) plus the fp32 error of a K-term sum, one fmaf and one
add (each at most 2^-24 relative to the magnitude sum).  The bar is derived, not measured.

Stem pooling (convnets/infer.affine_relu_maxpool = dle_bn_relu_maxpool_fwd with (mean, rstd, gamma, beta) = (0, scale, 1, shift)):
exact-grid inputs, float64 affine + ReLU + MaxPool2d(3, 2, 1) on the CPU, bits; (2,16,16,64) and the real (1,112,112,64).

Outputs are views at the head of over-long NaN-filled buffers: the tail must keep its bits.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from deeplearningexamples_amd.convnets.infer import affine_relu_maxpool
from tests._exact_grid import B_MFMA, Out, assert_same, bits, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
F64 = torch.float64
DEV = "cuda"

# name -> (N, H, W, C, Ko, R, stride, pad, halo launches per call)
SHAPES = {
    "halo_2x14x14_64_64": (2, 14, 14, 64, 64, 3, 1, 1, 1),
    "halo_1x12x20_128_128": (1, 12, 20, 128, 128, 3, 1, 1, 1),
    "halo_5x10x10_64_192": (5, 10, 10, 64, 192, 3, 1, 1, 1),
    "mat_98x64x256": (2, 7, 7, 64, 256, 1, 1, 0, 0),
    "mat_392x256x64": (2, 14, 14, 256, 64, 1, 1, 0, 0),
    "mat_49x2048x512": (1, 7, 7, 2048, 512, 1, 1, 0, 0),
    "im2col_1x1s2_256_512": (2, 14, 14, 256, 512, 1, 2, 0, 0),
    "im2col_3x3s2_128_128": (2, 14, 14, 128, 128, 3, 2, 1, 0),
    "im2col_3x3s1_7x7_512": (1, 7, 7, 512, 512, 3, 1, 1, 0),
}
COMBOS = [pytest.param(res, relu, id=("res" if res else "nores") + ("+relu" if relu else "")) for res in (False, True)
          for relu in (False, True)]


def ref_conv(x, w, stride, pad):
    """[N, P, Q, Ko] float64 of x [N, H, W, C], w [Ko, R, S, C]: a sum of per-tap matrix products."""
    x, w = x.to(F64), w.to(F64)
    n, h, wd, c = x.shape
    ko, r, s, _ = w.shape
    p, q = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros((n * p * q, ko), dtype=F64, device=x.device)
    for i in range(r):
        for j in range(s):
            win = xp[:, i:i + stride * (p - 1) + 1:stride, j:j + stride * (q - 1) + 1:stride, :]
            y.addmm_(win.reshape(-1, c), w[:, i, j, :].t())
    return y.view(n, p, q, ko)


def launches():
    return int(C.lib().dle_conv3x3_affine_launch_count())


def run(case, x, w, scale, shift, res, relu):
    n, h, wd, c, ko, r, stride, pad, halo = SHAPES[case]
    p, q = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - r) // stride + 1
    out = Out((n, p, q, ko), x.dtype, DEV)
    before = launches()
    F.conv2d_fwd_affine(x, w, scale, shift, stride, pad, residual=res, relu=relu, out=out.t)
    torch.cuda.synchronize()
    assert launches() - before == halo, "%s: the halo-tile kernel %s" % (case, "declined the shape" if halo else "took a shape outside its envelope")
    return out.check(case)


# ---------------------------------------------------------------- bit-exact cases
@functools.lru_cache(maxsize=None)
def exact_case(case, dtype):
    n, h, wd, c, ko, r, stride, pad, _ = SHAPES[case]
    seed = sum(map(ord, case)) + (1 if dtype == HF else 0)
    x = grid((n, h, wd, c), seed, dtype, DEV)
    w = grid((ko, r, r, c), seed + 1, dtype, DEV)
    g = gen(DEV, seed + 2)
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV)[torch.randint(0, 6, (ko,), generator=g, device=DEV)]
    shift = torch.randint(-64, 65, (ko,), generator=g, device=DEV).float() / 16
    acc = ref_conv(x, w, stride, pad)
    mag = ref_conv(x.abs(), w.abs(), stride, pad)
    assert float(mag.max()) < B_MFMA, "contraction magnitude sum %g: the fp32 accumulator would not be exact" % float(mag.max())
    res = grid(tuple(acc.shape), seed + 3, dtype, DEV)
    return x, w, scale, shift, res, acc


@pytest.mark.parametrize("with_res,relu", COMBOS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_exact_grid_bits(case, dtype, with_res, relu):
    x, w, scale, shift, res, acc = exact_case(case, dtype)
    pre = scale.to(F64) * acc + shift.to(F64)
    if with_res:
        pre = pre + res.to(F64)
    assert torch.equal(pre * 32, torch.round(pre * 32)), "pre-rounding value off the 1/32 grid"
    assert float(pre.abs().max()) < 2.0 ** 19, "pre-rounding value too large to be exact in fp32"
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    if relu:
        assert bool((pre < 0).any()), "the ReLU clips nothing in this case"
        pre = pre.clamp_min(0)
    want = pre.float().to(dtype)
    got = run(case, x, w, scale, shift, res if with_res else None, relu)
    assert_same(bits(got), bits(want), "%s %s res=%d relu=%d" % (case, dtype, with_res, relu))


# ---------------------------------------------------------------- random inputs, per-element derived bar
@functools.lru_cache(maxsize=None)
def random_case(case, dtype):
    n, h, wd, c, ko, r, stride, pad, _ = SHAPES[case]
    g = gen(DEV, 1000 + sum(map(ord, case)) + (1 if dtype == HF else 0))
    k = r * r * c
    x = torch.randn((n, h, wd, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, r, r, c), generator=g, device=DEV) / k ** 0.5).to(dtype)
    scale = (0.25 + 3.75 * torch.rand((ko,), generator=g, device=DEV)) * (torch.randint(0, 2, (ko,), generator=g, device=DEV) * 2 - 1).float()
    shift = torch.randn((ko,), generator=g, device=DEV)
    acc = ref_conv(x, w, stride, pad)
    mag = ref_conv(x.abs(), w.abs(), stride, pad)
    res = torch.randn(tuple(acc.shape), generator=g, device=DEV).to(dtype)
    return x, w, scale, shift, res, acc, mag


@pytest.mark.parametrize("with_res,relu", COMBOS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_random_inputs_per_element_bar(case, dtype, with_res, relu):
    x, w, scale, shift, res, acc, mag = random_case(case, dtype)
    terms = SHAPES[case][5] ** 2 * SHAPES[case][3]
    ref = scale.to(F64) * acc + shift.to(F64)
    budget = scale.to(F64).abs() * mag + shift.to(F64).abs()
    if with_res:
        ref = ref + res.to(F64)
        budget = budget + res.to(F64).abs()
    if relu:
        ref = ref.clamp_min(0)
    got = run(case, x, w, scale, shift, res if with_res else None, relu).to(F64)
    bar = ulp16(ref, dtype) / 2 + (terms + 3) * 2.0 ** -24 * budget
    err = (got - ref).abs()
    worst = float((err / bar).max())
    print("%s %s res=%d relu=%d: max err %.3e, max err / bar %.3f" % (case, dtype, with_res, relu, float(err.max()), worst))
    assert bool(torch.isfinite(got).all())
    bad = err > bar
    assert not bool(bad.any()), "%d of %d elements above the bar, worst err / bar %.3f" % (int(bad.sum()), bad.numel(), worst)


# ---------------------------------------------------------------- argument checks (no launch)
def test_rejects_misaligned_and_fp32():
    x = torch.zeros((1, 8, 8, 64), dtype=BF, device=DEV)
    w = torch.zeros((64, 1, 1, 64), dtype=BF, device=DEV)
    sc = torch.ones(68, device=DEV)
    with pytest.raises(ValueError):
        F.conv2d_fwd_affine(x, w, sc[1:65], sc[:64])                     # scale not 16-byte aligned (and not [Ko] storage)
    with pytest.raises(ValueError):
        F.conv2d_fwd_affine(x.float(), w.float(), sc[:64], sc[:64])       # 16-bit dtypes only
    with pytest.raises(ValueError):
        F.conv2d_fwd_affine(x, w, sc[:64], sc[:64], residual=torch.zeros((1, 8, 8, 32), dtype=BF, device=DEV))


# ---------------------------------------------------------------- the stem's pooling pass
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (1, 112, 112, 64)], ids=["2x16x16", "1x112x112"])
def test_stem_affine_relu_maxpool_bits(shape, dtype):
    n, h, wd, c = shape
    t = grid(shape, 77, dtype, DEV)
    g = gen(DEV, 78)
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV)[torch.randint(0, 6, (c,), generator=g, device=DEV)]
    shift = torch.randint(-16, 17, (c,), generator=g, device=DEV).float() / 16
    got = affine_relu_maxpool(t, scale, shift, torch.zeros_like(scale), torch.ones_like(scale))     # as ResNet50Classifier._stem calls it
    torch.cuda.synchronize()
    pre = (t.cpu().to(F64) * scale.cpu().to(F64) + shift.cpu().to(F64)).clamp_min(0)          # exact: multiples of 1/16 below 4
    assert torch.equal(pre * 16, torch.round(pre * 16)) and bool((pre == 0).any())
    want = torch.nn.functional.max_pool2d(pre.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).float().to(dtype)
    assert tuple(got.shape) == (n, h // 2, wd // 2, c)
    assert_same(bits(got.cpu()), bits(want.contiguous()), "stem pool %s %s" % (shape, dtype))
