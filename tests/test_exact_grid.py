"""CPU self-test of tests/_exact_grid.py, the helpers the bit-exact float64-reference tests rest on: if grid() stopped being exactly
summable, or the comparison stopped seeing one wrong term, every such GPU test would pass while checking nothing."""
import pytest
import torch

from tests._exact_grid import B_MFMA, Out, assert_same, bits, check_exact, grid, ulp16

CPU = torch.device("cpu")
TYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dtype", TYPES, ids=["fp16", "bf16"])
def test_grid_round_trip(dtype):
    """k / 4 with |k| <= 4 is exact in both 16-bit types, the density thins it, and every value is on the grid."""
    g32 = grid((4096,), 3, torch.float32, CPU)
    g16 = grid((4096,), 3, dtype, CPU)
    assert torch.equal(g16.float(), g32) and torch.equal(g32.to(dtype).float(), g32)
    assert torch.equal(g32 * 4, torch.round(g32 * 4)) and float(g32.abs().max()) == 1.0
    assert set((g32 * 4).long().tolist()) == set(range(-4, 5))
    thin = grid((4096,), 3, dtype, CPU, kmax=2, density=0.5)
    assert float(thin.float().abs().max()) == 0.5 and 0.3 < float((thin == 0).float().mean()) < 0.8


@pytest.mark.parametrize("dtype", TYPES, ids=["fp16", "bf16"])
def test_fp32_product_is_exact_and_one_wrong_term_shows(dtype):
    """300 x 64 x 4096: the fp32 product equals the float64 one bit for bit (whatever order the CPU library adds in), the bound is
    met from the data, and one operand element moved by 1/4 breaks the equality."""
    a = grid((300, 4096), 11, dtype, CPU)
    b = grid((64, 4096), 12, dtype, CPU)
    worst = float((a.double().abs() @ b.double().abs().T).max())
    assert worst < B_MFMA and worst * 16 < 2 ** 24
    ref = a.double() @ b.double().T
    check_exact(ref)
    got = a.float() @ b.float().T
    assert_same(got, ref.float(), "fp32 product")
    assert torch.equal(got.double(), ref)
    assert_same(got.to(dtype), ref.float().to(dtype), "rounded once")
    a2 = a.clone()
    a2[17, 1234] += 0.25
    bad = a2.float() @ b.float().T
    with pytest.raises(AssertionError, match="elements differ"):
        assert_same(bad, ref.float(), "one element moved by 1/4")
    assert int((bad != ref.float()).sum()) == int((b[:, 1234] != 0).sum())
    with pytest.raises(AssertionError):
        check_exact(ref + 1.0 / 32)
    with pytest.raises(AssertionError):
        check_exact(ref.abs() * 4096)


@pytest.mark.parametrize("dtype", TYPES, ids=["fp16", "bf16"])
def test_ulp16_is_the_spacing(dtype):
    pts = [1.0, 1.5, 0.75, 3.0, 100.0, 2.0 ** -10, 1000.0, 6e-5]
    for p in pts:
        v = torch.tensor(p, dtype=dtype)
        up = torch.nextafter(v, torch.tensor(float("inf"), dtype=dtype))
        assert float(ulp16(v.double(), dtype)) == float(up.double() - v.double()), p
        assert float(ulp16(-v.double(), dtype)) == float(up.double() - v.double()), p
    tiny = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}[dtype]
    assert float(ulp16(torch.zeros((), dtype=torch.float64), dtype)) == tiny
    assert float(ulp16(torch.tensor(tiny * 3, dtype=torch.float64), dtype)) == tiny


def test_out_guard_sees_a_stray_write_and_a_hole():
    o = Out((5, 7), torch.float32, CPU)
    assert bool(torch.isnan(o.t).all())
    o.t.zero_()
    assert_same(o.check("ok"), torch.zeros(5, 7), "filled")
    o.buf[35] = 1.0
    with pytest.raises(AssertionError, match="past the end"):
        o.check("stray")
    h = Out((4,), torch.bfloat16, CPU)
    h.t[:3] = 1.0
    with pytest.raises(AssertionError):
        assert_same(h.check("hole"), torch.ones(4, dtype=torch.bfloat16), "a NaN left inside")
    b = Out((16,), torch.uint8, CPU)
    assert int(b.t[0]) == 0xFF and bits(b.buf).dtype == torch.uint8
    b.buf[16] = 0
    with pytest.raises(AssertionError, match="past the end"):
        b.check("bits")
