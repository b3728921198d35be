"""Exactly summable test inputs (tests/ only), shared by the float64-reference tests of the ResNet-50 kernels.

Values k / 4 with small integer k are exact in fp16 and bf16, every product of two of them is a multiple of 1/16, and while the
sum of the magnitudes of the terms of a sum stays below a bound B every partial sum, in any order, is a multiple of 1/16 below B:
with B <= 2^20 it has at most 24 significant bits, so the fp32 sum is EXACT whatever order a kernel adds in."""
import math

import torch

# Bound on the sum of magnitudes for sums that run through the matrix units (not the 2^20 of plain fp32 additions): headroom for a
# matrix unit that aligns a group of products to the largest exponent before it adds them.
B_MFMA = 2.0 ** 18
TAIL = 4096


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def grid(shape, seed, dtype, dev, kmax=4, density=1.0):
    """k / 4 with |k| <= kmax: exact in fp16 and bf16, squares and products of two multiples of 1/16.  density < 1 zeroes the
    other entries (a smaller sum of magnitudes for the long contractions)."""
    g = gen(dev, seed)
    k = torch.randint(-kmax, kmax + 1, shape, generator=g, device=dev)
    if density < 1.0:
        k = k * (torch.rand(shape, generator=g, device=dev) < density)
    return (k.float() * 0.25).to(dtype)


def check_exact(*terms, bound=2.0 ** 20):
    """Precondition of the bit-exact bars: every term [M, C] (float64) is a multiple of 1/16 and each column's sum of magnitudes is
    below `bound`, so every partial sum, in any order, is a multiple of 1/16 below it: at most 24 significant bits, exact in fp32."""
    for t in terms:
        assert torch.equal(t * 16, torch.round(t * 16)), "term off the 1/16 grid"
        worst = float(t.abs().sum(0).max())
        assert worst < bound, "column magnitude sum %g: fp32 sums would not be exact" % worst


MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


def ulp16(v, dtype):
    """Spacing of `dtype` at |v| (float64), the subnormal spacing at and near 0."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype])


def bits(t):
    """The tensor's storage as integers of its element size (NaN payloads and signed zeros compare as bits)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_same(got, want, what):
    if torch.equal(got, want):
        return
    bad = got != want
    idx = torch.nonzero(bad)[:4]
    first = tuple(idx[0].tolist())
    raise AssertionError("%s: %d of %d elements differ, first at %s (got %r, want %r); more at %s" % (
        what, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first]), idx[1:].tolist()))


class Out:
    """An output as a view at the head of an over-long buffer filled with NaN (0xFF bytes for integer types), or holding `fill`
    in the view: the tail must keep its bits."""

    def __init__(self, shape, dtype, dev, fill=None):
        self.n = math.prod(shape)
        if dtype.is_floating_point:
            self.buf = torch.full((self.n + TAIL,), float("nan"), dtype=dtype, device=dev)
        else:
            self.buf = torch.full((self.n + TAIL,), 0xFF, dtype=dtype, device=dev)
        self.t = self.buf[:self.n].view(shape)
        if fill is not None:
            self.t.copy_(fill)
        self.tail = bits(self.buf[self.n:]).clone()

    def check(self, what):
        assert torch.equal(bits(self.buf[self.n:]), self.tail), "%s wrote past the end of its output" % what
        return self.t
