"""dle_se_gate / dle_se_apply -- squeeze-and-excitation for the SE-ResNeXt inference path (csrc/se.hip) -- against float64.
GPU only.

se_apply, exact.  y = round16(relu?(fmaf(t, gate[n,c], residual))).  t and the residual are k / 4 with |k| <= 4, the gates powers of
two in [1/8, 1]: t * gate + residual is a multiple of 1/32 of magnitude at most 2, exact in fp32, so the output is the float64 value
rounded once: bits are compared.  ReLU on and off (the ReLU cases assert that something was clipped), with and without a residual,
at (N, HW, C) = (2, 4, 256), (3, 49, 2048), (1, 3136, 256).

se_gate, against float64 with a propagated bar (u = 2^-24; m, z1, h, z2 the float64 values):
    |d mean| <= (HW + 1) u mean|t|                                  a HW-term fp32 sum and the scaling by 1 / HW
    |d z1|   <= (C + 2) u (sum|w1||m| + |b1|) + sum|w1| |d mean|    a C-term fp32 dot product + bias, and the propagated error
    |d h|    <= |d z1|                                              ReLU is 1-Lipschitz
    |d z2|   <= (S + 2) u (sum|w2||h| + |b2|) + sum|w2| |d h|
    |d gate| <= |d z2| / 4 + c u                                    sigmoid' <= 1/4; c u: the device's exponential and division
c is not derived: it is measured here, on the device, as max |torch.sigmoid(z_fp32) - sigmoid64(z)| / u over a dense grid of z in
[-30, 30] -- torch's kernel, not the one under test -- and the bar allows twice that value, because two independent expf
implementations may each be off by their own unit.  The measured value is printed (DESIGN.md section 4i records it).
Shapes (N, HW, C, S): (2, 4, 256, 16), (1, 3136, 256, 16), (3, 49, 2048, 16), (2, 16, 512, 8).

Outputs are views at the head of over-long NaN-filled buffers: the tail must keep its bits.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from tests._exact_grid import Out, assert_same, bits, gen, grid

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
F64 = torch.float64
DEV = "cuda"
U = 2.0 ** -24


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 4, 256), (3, 49, 2048), (1, 3136, 256)], ids=lambda s: "x".join(map(str, s)))
def test_se_apply_exact_bits(shape, dtype, relu, res):
    n, hw, c = shape
    t = grid(shape, 31, dtype, DEV)
    r = grid(shape, 32, dtype, DEV) if res else None
    gate = torch.pow(2.0, -torch.randint(0, 4, (n, c), generator=gen(DEV, 33), device=DEV).float())
    assert float(gate.min()) >= 0.125 and float(gate.max()) <= 1.0
    pre = t.double() * gate.double()[:, None, :] + (r.double() if res else 0.0)
    assert torch.equal(pre * 32, torch.round(pre * 32)) and float(pre.abs().max()) <= 2.0
    want = pre
    if relu:
        assert bool((pre < 0).any()), "nothing for the ReLU to clip"
        want = pre.clamp_min(0)
    o = Out(shape, dtype, DEV)
    y = F.se_apply(t, gate, residual=r, relu=relu, out=o.t)
    assert y.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    assert_same(bits(o.check("se_apply")), bits(want.float().to(dtype)), "se_apply %s %s" % (shape, dtype))


@functools.lru_cache(maxsize=None)
def sigmoid_units():
    """c: max |torch.sigmoid(z_fp32) - sigmoid64(z)| / u over a dense grid of z in [-30, 30], on the device."""
    z = torch.linspace(-30.0, 30.0, 2000001, dtype=F64, device=DEV).float()
    z = torch.cat([z, torch.randn(1000000, generator=gen(DEV, 41), device=DEV) * 3])
    err = (torch.sigmoid(z).double() - torch.sigmoid(z.double())).abs()
    return float(err.max()) / U


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 4, 256, 16), (1, 3136, 256, 16), (3, 49, 2048, 16), (2, 16, 512, 8)],
                         ids=lambda s: "x".join(map(str, s)))
def test_se_gate_against_float64(shape, dtype):
    n, hw, c, s = shape
    g = gen(DEV, 51)
    t = torch.randn((n, hw, c), generator=g, device=DEV).to(dtype)
    w1 = torch.randn((s, c), generator=g, device=DEV) * c ** -0.5
    b1 = torch.randn((s,), generator=g, device=DEV) * 0.1
    w2 = torch.randn((c, s), generator=g, device=DEV) * s ** -0.5 * 2
    b2 = torch.randn((c,), generator=g, device=DEV) * 0.1
    o = Out((n, c), torch.float32, DEV)
    got = F.se_gate(t, w1, b1, w2, b2, out=o.t)
    assert got.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    got = o.check("se_gate").double()
    t64, w1d, b1d, w2d, b2d = t.double(), w1.double(), b1.double(), w2.double(), b2.double()
    m = t64.mean(1)                                                     # [n, c]
    d_mean = (hw + 1) * U * t64.abs().mean(1)
    z1 = m @ w1d.t() + b1d
    d_z1 = (c + 2) * U * (m.abs() @ w1d.abs().t() + b1d.abs()) + d_mean @ w1d.abs().t()
    h = z1.clamp_min(0)
    z2 = h @ w2d.t() + b2d
    d_z2 = (s + 2) * U * (h @ w2d.abs().t() + b2d.abs()) + d_z1 @ w2d.abs().t()
    ref = torch.sigmoid(z2)
    cu = sigmoid_units()
    assert 0 < cu < 16, cu                                              # a sane yardstick
    bar = d_z2 / 4 + 2 * cu * U
    err = (got - ref).abs()
    print("se_gate %s %s: sigmoid yardstick c = %.3f u; max err %.3e, max err / bar %.3f; gate range [%.3f, %.3f]" % (
        shape, dtype, cu, float(err.max()), float((err / bar).max()), float(ref.min()), float(ref.max())))
    assert bool(torch.isfinite(got).all())
    assert float(ref.max()) - float(ref.min()) > 0.2                    # the gates are not all alike
    assert bool((err <= bar).all()), "%d of %d gates over the bar" % (int((err > bar).sum()), err.numel())


def test_argument_checks():
    t = torch.zeros((1, 4, 64), dtype=BF, device=DEV)
    with pytest.raises(ValueError):                                     # hidden width above 64
        F.se_gate(t, torch.zeros((65, 64), device=DEV), torch.zeros(65, device=DEV), torch.zeros((64, 65), device=DEV),
                  torch.zeros(64, device=DEV))
    with pytest.raises(ValueError):                                     # fp32 activations
        F.se_apply(t.float(), torch.ones((1, 64), device=DEV))
    with pytest.raises(ValueError):                                     # C not a multiple of 8
        F.se_apply(torch.zeros((1, 4, 12), dtype=BF, device=DEV), torch.ones((1, 12), device=DEV))
    torch.cuda.synchronize()
