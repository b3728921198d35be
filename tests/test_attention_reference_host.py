"""CPU-only checks of tests/_attention_reference.py (the float64 statement, exact inputs and bars the GPU test holds the fused
attention kernels of csrc/attention.hip to).

1. The closed-form float64 forward / backward equals torch autograd in float64 (p = 0 and a random keep mask).
2. Every constructor of exactly computable inputs meets its preconditions at every shape the GPU test runs (the constructors
   assert them: score gap >= 104, magnitude sums below B_MFMA, dS with at most 8 significant bits, delta = 0, ...).
3. A CPU model of the kernels' arithmetic (fp32 softmax, dropout(P) and dS rounded once to 16 bits, fp32 sums in two orders,
   blocked online max / sum above S = 128) gives the SAME BITS as the float64 expectation on the exact inputs and stays inside
   the per-element and per-block bars on the generic inputs; the float64 reference rounded once passes its own bars.
   Largest |model - ref| / bar over all generic cases (test_zz_report with -s prints them):
       per element   ctx 0.836  dq 0.903  dk 0.771  dv 0.922    row max 0.257  1 / row sum 0.153
       per block L2  ctx 0.678  dq 0.350  dk 0.343  dv 0.340    (bars 2^-(m+1) for ctx, 2 x 2^-(m+1) for the gradients)
   Under the short form of the bars (no subnormal operand spacing, no error of dP / delta, row max within 2 u (1 + |max|); see
   the GPU file) the same model reaches ctx 11.7, dq 10.5, dk 5.7, dv 2.4, row max 1.3: recorded as lit_*, not asserted.
4. Planted errors in that model leave the bars: keys 1 and 2 of an 8-key chunk exchanged, a key block skipped in pass 2, the two
   4-float halves of the mask's 8-key groups exchanged, the dropout chunk index off by one row at S = 1024, a stale row max (the
   online rescale omitted), P rounded before instead of after the dropout scale -- each caught by an exact case AND by the generic
   bars.  (The exact case for the last one: P = 1 / n, n not a power of two, p = 0.1 -- the two roundings store different bits
   while everything else stays exact.)
"""
import pytest
import torch

from tests import _attention_reference as A

SEED, OFF = 0x1234567887654321, (1 << 34) + 9
RATIOS = {}


def _keep(s, b, nh, p):
    return A.oracle_keep(b, nh, s, p, SEED, OFF) if p > 0 else None


def _model(inputs, s, b, nh, scale, p, order=0, fault=None):
    qkv, dctx, mask_add = inputs
    return A.kernel_model(qkv, dctx, mask_add, _keep(s, b, nh, p), b, s, nh, scale, A.inv_keep(p), order, fault)


def _io(case):
    return case.qkv, case.dctx, case.mask_add


# ------------------------------------------------------------------------------------------------ 1. closed form == autograd
@pytest.mark.parametrize("with_keep", [False, True], ids=["p0", "keep"])
def test_reference_matches_autograd(with_keep):
    b, s, nh = 2, 24, 2
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b * s, 3 * nh * A.D, generator=g, dtype=torch.float64)
    dctx = torch.randn(b * s, nh * A.D, generator=g, dtype=torch.float64)
    mask = torch.where(torch.rand(b, s, generator=g) < 0.3, A.NEG, 0.0)
    keep = (torch.rand(b, nh, s, s, generator=g) < 0.8) if with_keep else None
    ik, scale = 1.25 if with_keep else 1.0, 0.125
    r = A.reference(qkv, dctx, mask, keep, b, s, nh, scale, ik)
    x = qkv.clone().requires_grad_(True)
    q, k, v = A.split(x, b, s, nh)
    P = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale + mask.double()[:, None, None, :], -1)
    Pd = P if keep is None else torch.where(keep, P * ik, torch.zeros((), dtype=torch.float64))
    ctx = torch.matmul(Pd, v)
    ctx.backward(A.heads(dctx, b, s, nh))
    dq, dk, dv = A.split(x.grad, b, s, nh)
    for nm, want in (("ctx", ctx.detach()), ("dq", dq), ("dk", dk), ("dv", dv), ("P", P.detach())):
        assert float((r[nm] - want).abs().max()) <= 1e-13 * (1.0 + float(want.abs().max())), nm


# ------------------------------------------------------------------------------------------------ 2 + 3. exact inputs
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_selector_model_exact(shape, dtype):
    s, b, nh = shape
    case = A.Selector(s, b, nh, dtype, with_mask=b > 1)            # (the constructor asserts its preconditions)
    r = A.reference(case.qkv, case.dctx, case.mask_add, None, b, s, nh, case.scale, 1.0)
    exp = case.expected(None, 1.0)
    for nm in ("ctx", "dq", "dk", "dv"):      # the closed-form expectation is the float64 statement up to exp(-128) = 2.6e-56
        assert float((r[nm] - exp[nm]).abs().max()) < 1e-50, nm                      # (not 0 in float64; exactly 0 in fp32)
    assert float((r["P"] * (1 - r["P"])).abs().max()) < 1e-50 and float((r["inv"] - 1).abs().max()) < 1e-50
    for p in (0.0, 0.5):
        for order in (0, 1):
            out = _model(_io(case), s, b, nh, case.scale, p, order)
            A.check_selector(out, case, _keep(s, b, nh, p), A.inv_keep(p), "model order %d p %g" % (order, p))
            A.check_colsum(torch.cat([A.merge(out[nm]) for nm in ("dq", "dk", "dv")], 1).double(), "selector")


def test_selector_preconditions_big():
    s, b, nh = A.BIG
    for dtype in A.DTYPES:
        A.Selector(s, b, nh, dtype)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("mirror", [False, True], ids=["q0", "k0"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_uniform_model_exact(shape, mirror, dtype):
    s, b, nh = shape
    assert A.inv_keep(0.5) == 2.0
    for plan in A.PLANS[shape]:
        case = A.Uniform(s, b, nh, dtype, plan, mirror)
        for order in (0, 1):
            out = _model(_io(case), s, b, nh, case.scale, 0.0, order)
            A.check_uniform_fwd(out, case, None, 1.0, "model order %d" % order)
            r = A.check_uniform_bwd(out, case, "model order %d" % order)           # (asserts delta = 0, dS exact, the sums)
            assert float(r["ctx"].abs().max()) > 0 and float(r["dv"].abs().max()) > 0
            if plan != [1]:                                        # (one valid key: the softmax has no gradient)
                assert float((r["dk"] if mirror else r["dq"]).abs().max()) > 0
            A.check_colsum(torch.cat([A.merge(out[nm]) for nm in ("dq", "dk", "dv")], 1).double(), "uniform")
            out = _model(_io(case), s, b, nh, case.scale, 0.5, order)              # p = 0.5: the forward pass is exact,
            keep = _keep(s, b, nh, 0.5)
            A.check_uniform_fwd(out, case, keep, 2.0, "model order %d p 0.5" % order)
            rr = A.reference(case.qkv, case.dctx, case.mask_add, keep, b, s, nh, case.scale, 2.0)
            A.check_generic({k: out[k] for k in ("dq", "dk", "dv")}, rr, dtype, "uniform p 0.5")   # the backward under the bars


# ------------------------------------------------------------------------------------------------ 3. generic inputs
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("sigma", [0.8, 3.0])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_model_inside_generic_bars(shape, sigma, p, dtype):
    s, b, nh = shape
    inp = A.generic_inputs(s, b, nh, dtype, sigma)
    keep, ik = _keep(s, b, nh, p), A.inv_keep(p)
    r = A.reference(*inp, keep, b, s, nh, 0.125, ik)
    own = {k: A.r16(r[k], dtype) for k in ("ctx", "dq", "dk", "dv")}
    own.update(mx=r["mx"], inv=r["inv"])
    A.check_generic(own, r, dtype, "the reference rounded once")
    for order in (0, 1):
        A.check_generic(_model(inp, s, b, nh, 0.125, p, order), r, dtype, "model order %d" % order, RATIOS)


# ------------------------------------------------------------------------------------------------ 4. planted errors
def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _exact_selector(shape, p, fault, dtype):
    s, b, nh = shape
    case = A.Selector(s, b, nh, dtype, with_mask=b > 1)
    out = _model(_io(case), s, b, nh, case.scale, p, 0, fault)
    return _caught(lambda: A.check_selector(out, case, _keep(s, b, nh, p), A.inv_keep(p), str(fault)))


def _generic(shape, p, fault, dtype, sigma=3.0):
    s, b, nh = shape
    inp = A.generic_inputs(s, b, nh, dtype, sigma)
    keep, ik = _keep(s, b, nh, p), A.inv_keep(p)
    r = A.reference(*inp, keep, b, s, nh, 0.125, ik)
    return _caught(lambda: A.check_generic(_model(inp, s, b, nh, 0.125, p, 0, fault), r, dtype, str(fault)))


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("fault,shape,p", [("swap_keys", (128, 1, 1), 0.0), ("skip_block", (256, 2, 3), 0.0),
                                           ("chunk_row", (1024, 1, 2), 0.5), ("stale_max", (384, 2, 2), 0.0)])
def test_planted_error_selector(fault, shape, p, dtype):
    assert not _exact_selector(shape, p, None, dtype)
    assert _exact_selector(shape, p, fault, dtype), "the selector case does not catch " + fault


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_planted_error_mask_halves_uniform(dtype):
    s, b, nh = 128, 3, 3
    case = A.Uniform(s, b, nh, dtype, A.PLANS[(s, b, nh)][0])
    for fault, want in ((None, False), ("mask_halves", True)):
        out = _model(_io(case), s, b, nh, case.scale, 0.0, 0, fault)
        assert _caught(lambda: A.check_uniform_fwd(out, case, None, 1.0, "")) == want
        assert _caught(lambda: A.check_uniform_bwd(out, case, "")) == want


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_planted_error_round_before_scale(dtype):
    """P = 1 / n with n not a power of two and p = 0.1: fp32 1 / n times fp32 inv_keep rounded once is NOT the 16-bit 1 / n times
    inv_keep rounded again; everything else (exp(0) = 1, a sum of n ones, the correctly rounded division, the products P16 x V on
    a grid) is exact, so the forward pass is still bit-comparable."""
    s, b, nh, p = 128, 1, 1, 0.1
    ik = A.inv_keep(p)
    case = A.Uniform(s, b, nh, dtype, [A.odd_n(dtype, ik)], pair=False)
    keep = _keep(s, b, nh, p)
    for fault, want in ((None, False), ("round_before", True)):
        out = _model(_io(case), s, b, nh, case.scale, p, 0, fault)
        assert _caught(lambda: A.check_uniform_fwd(out, case, keep, ik, "")) == want
    assert _generic((128, 3, 3), 0.1, "round_before", dtype), "the generic bars do not catch round_before"


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("fault,shape,p", [("swap_keys", (128, 3, 3), 0.0), ("skip_block", (256, 2, 3), 0.0),
                                           ("mask_halves", (256, 2, 3), 0.0), ("chunk_row", (1024, 1, 2), 0.1),
                                           ("stale_max", (384, 2, 2), 0.0)])
def test_planted_error_generic(fault, shape, p, dtype):
    assert not _generic(shape, p, None, dtype)
    assert _generic(shape, p, fault, dtype), "the generic bars do not catch " + fault


def test_zz_report():
    print("\nlargest |model - ref| / bar: " + "  ".join("%s %.3f" % kv for kv in sorted(RATIOS.items())))
