"""Proof of tests/_bnconv_reference.py on the CPU: its comparison functions against an fp32 torch MODEL of each kernel's arithmetic
(csrc/conv_bnload.hip, csrc/conv_bnbwd.hip, csrc/gemm_expand.hip with the bnred epilogue), at a few hundred rows.

The honest model rounds where the kernels round (fp32 coefficients, fp32 apply chain, one rounding to 16 bits, fp32 products and
sums of the ROUNDED values, 1 / M in fp32) and must
* pass every exact case bit for bit (M = 256, a power of two, and M = 357 = 5 x 64 + 37 with its half-and-half channels), and
* stay below a stated fraction of each Gaussian bar.  Measured here (worst over shapes, residual modes and both dtypes):
      16-bit outputs (y, dt, out, dx): the whole bar is reached (1.00): a rounding tie sits exactly on ulp16 / 2, its first
      term.  What counts is the error PAST that half step as a fraction of the REST of the bar ("fp32 term"): out 0.017, dx 0.005,
      dx of the bnred GEMM 0.020, dt 0.253, y 0.207 without the branch BatchNorm.  Where the rest carries a tie term (a whole
      16-bit step of the residual or of a dt near a rounding boundary, taken in full or not at all) it is used up almost entirely
      when taken: y with the branch BatchNorm 0.956, dx of the weight-gradient form 0.645, gw of that form 0.72;
      fp32 sums and what follows from them: S0 0.006, S1 0.015, dbeta2 0.001, dgamma2 0.004, mean 0.006, rstd 0.013,
      running_mean 0.125, running_var 0.113 (the chain length handed in is n = M, generous for torch's pairwise sums).
  FRACTION below states 0.3 for an fp32 term without a tie, 0.25 for the sums and 1.0 where a tie term is part of the bar.
Each planted fault must be rejected, in the exact kind and in the Gaussian kind (two of them are planted in the Gaussian kind only,
see test_bnload_fault):
  kb and kg swapped; 1 / M from the padded row count; keep bits read (or written) most significant bit first; the last partial row
  tile dropped; a poisoned row past M entering gw or a reduction; statistics of the unrounded out; mean2 of the wrong column block;
  the branch-BatchNorm residual not rounded to 16 bits before the add.
That is the evidence that the bars are tight enough to matter and loose enough for correct code.  The chain lengths n handed to
the comparisons are those of the model's own summation (torch's fp32 sums over at most 357 rows and its blocked matmul): n = M."""
import types

import pytest
import torch

from tests import _bnconv_reference as R

BF, HF = torch.bfloat16, torch.float16
DT_IDS = {BF: "bf16", HF: "fp16"}
CPU = torch.device("cpu")
TM = 64
M_POW2, M_RAGGED = 256, 5 * TM + 37
FRACTION = {"fp32 term": 0.3, "32": 0.25, "tie": 1.0}
SUMS32 = ("S0", "S1", "mean", "rstd", "running_mean", "running_var", "dbeta2", "dgamma2")


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype)


def _unpack_msb(bits, shape):
    b = (bits.to(torch.int32).unsqueeze(1) >> (7 - torch.arange(8, dtype=torch.int32))) & 1
    return b.reshape(shape).bool()


def _pack_msb(keep):
    b = keep.reshape(-1, 8).to(torch.int32) << (7 - torch.arange(8, dtype=torch.int32))
    return b.sum(1).to(torch.uint8)


def _live(m, fault):
    return m // TM * TM if fault == "drop_tile" else m


def _poison_row(c):
    return torch.full((1, c), R.POISON)


# ---------------------------------------------------------------- fp32 models
def model_bnload(s, w, fault=None):
    m, dt = s.m, s.dtype
    mean, rstd, gam, beta = s.bn
    sc = rstd * gam
    v = s.t.float() * sc + (beta - mean * sc)
    if s.resmode == 1:
        v = v + s.res.float()
    elif s.resmode == 2:
        mr, rr, gr, br = s.bnr
        scr = rr * gr
        r = s.res.float() * scr + (br - mr * scr)
        if fault != "res_unrounded":
            r = r.to(dt).float()
        v = v + r
    v = torch.where(v > 0, v, torch.zeros(()))
    live = _live(m, fault)
    got = types.SimpleNamespace(y=_nan((m, s.k), dt), out=_nan((m, s.n), dt))
    got.y[:live] = v[:live].to(dt)
    keep = torch.ones((m, s.k), dtype=torch.bool)
    keep[:live] = v[:live] > 0
    got.bits = _pack_msb(keep) if fault == "msb" else R.pack_bits(keep)
    out32 = got.y[:live].float() @ w.float().t()
    got.out[:live] = out32.to(dt)
    z = out32 if fault == "stats_unrounded" else got.out[:live].float()
    if fault == "poison_row":
        z = torch.cat([z, _poison_row(s.n)])
    s0, s1 = z.sum(0), (z * z).sum(0)
    got.S = torch.stack([s0, s1]).double()
    mean_o = got.S[0] / m
    var = (got.S[1] / m - mean_o * mean_o).clamp_min(0.0)
    got.mean, got.rstd = mean_o.float(), (1.0 / torch.sqrt(var + R.EPS64)).float()
    one_minus, mom = torch.tensor(1.0) - torch.tensor(R.MOM), torch.tensor(R.MOM)
    got.rm = one_minus * s.rm0 + mom * got.mean
    got.rv = one_minus * s.rv0 + mom * (var * m / (m - 1)).float()
    return got


def _sums2(s, dx_live, fault, roll):
    keep2 = s.keep2[:dx_live.shape[0]]
    mean2 = torch.roll(s.mean2, roll) if fault == "mean2_block" else s.mean2
    gz = dx_live.float() * keep2
    tx = gz * (s.t2[:dx_live.shape[0]].float() - mean2) * s.rstd2
    if fault == "poison_row":
        gz = torch.cat([gz, _poison_row(gz.shape[1])])
        tx = torch.cat([tx, _poison_row(gz.shape[1]) * (_poison_row(gz.shape[1]) - mean2) * s.rstd2])
    return gz.sum(0), tx.sum(0)


def model_bnbwd(s, wgform, fault=None):
    m, dt = s.m, s.dtype
    rows_for_m = -(-m // TM) * TM if fault == "padded_m" else m
    inv_m = torch.tensor(1.0) / torch.tensor(float(rows_for_m))
    kb, kg = s.dbeta * inv_m, s.dgamma * inv_m
    if fault == "swap":
        kb, kg = kg, kb
    g = s.dy.float()
    if s.masked:
        g = g * (_unpack_msb(s.bits, g.shape) if fault == "msb" else R.unpack_bits(s.bits, g.shape))
    xh = (s.t.float() - s.mean) * s.rstd
    dt16 = ((s.gamma * s.rstd) * (g - kb - xh * kg)).to(dt)
    live = _live(m, fault)
    got = types.SimpleNamespace(dt=None, dx=_nan((m, R.BN), dt))
    got.dx[:live] = (dt16[:live].float() @ s.w.float()).to(dt)
    if wgform:
        a, b = dt16[:live].float(), s.x[:live].float()
        if fault == "poison_row":
            a, b = torch.cat([a, _poison_row(R.BK)]), torch.cat([b, _poison_row(R.BN)])
        got.gw = a.t() @ b
    else:
        got.dt = _nan((m, R.BK), dt)
        got.dt[:live] = dt16[:live]
    if s.bred:
        got.db2, got.dg2 = _sums2(s, got.dx[:live], fault, 32)
    return got


def model_bnred(s, fault=None):
    m, dt = s.m, s.dtype
    keep1 = _unpack_msb(s.bits1, (m, s.n)) if fault == "msb" else s.keep1
    v = s.a.float() @ s.w.float() + torch.where(keep1, s.addend.float(), torch.zeros(()))
    live = _live(m, fault)
    got = types.SimpleNamespace(dx=_nan((m, s.n), dt))
    got.dx[:live] = v[:live].to(dt)
    got.db2, got.dg2 = _sums2(s, got.dx[:live], fault, 128)
    return got


# ---------------------------------------------------------------- the honest model
def _fractions(worst, tie=False):
    """tie: the case's 16-bit bars carry a tie term (branch BatchNorm, weight-gradient form)."""
    for name, ratio in worst.items():
        if name.endswith("fp32 term"):
            key = "tie" if tie and name.startswith(("y", "dx (wgrad form)")) else "fp32 term"
        elif name.startswith(SUMS32):
            key = "32"
        else:
            key = None                                       # whole 16-bit bars, gw's widened bar, the 1 ulp / 4 u bars: <= 1
        bound = 1.0 if key is None or "ulp" in name or "4u" in name else FRACTION[key]
        assert ratio <= bound, "%s: %g of its bar, stated fraction %g" % (name, ratio, bound)


BNLOAD = [(64, 64, 0), (64, 256, 1), (128, 128, 2), (256, 64, 1), (256, 128, 2), (256, 256, 0)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m", [M_POW2, M_RAGGED])
@pytest.mark.parametrize("k, n, resmode", BNLOAD)
def test_bnload_honest(k, n, resmode, m, dtype):
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnload_inputs(kind, dtype, CPU, m, k, n, resmode, 100 * k + n + resmode)
        what = "bnload %s %dx%dx%d res%d" % (kind, m, n, k, resmode)
        R.bnload_check(s, model_bnload(s, s.w), m, what, worst)
        if kind == "exact":
            R.bnload_check(s, model_bnload(s, s.w_dense), m, what, worst, dense=True)
    print("bnload", m, k, n, resmode, DT_IDS[dtype], worst)
    _fractions(worst, tie=resmode == 2)


BNBWD = [(masked, bred, wg) for masked in (True, False) for bred in (True, False) for wg in (False, True)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m", [M_POW2, M_RAGGED])
@pytest.mark.parametrize("masked, bred, wg", BNBWD)
def test_bnbwd_honest(masked, bred, wg, m, dtype):
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnbwd_inputs(kind, dtype, CPU, m, masked, bred, m + 2 * masked + bred)
        R.bnbwd_check(s, model_bnbwd(s, wg), {"bnred": m, "gw": m}, "bnbwd %s M=%d" % (kind, m), worst)
    print("bnbwd", m, masked, bred, wg, DT_IDS[dtype], worst)
    _fractions(worst, tie=wg)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m", [M_POW2, M_RAGGED])
@pytest.mark.parametrize("k, n", [(64, 128), (64, 256), (128, 256)])
def test_bnred_honest(k, n, m, dtype):
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnred_inputs(kind, dtype, CPU, m, k, n, 10 * k + n)
        R.bnred_check(s, model_bnred(s), m, "bnred %s %dx%dx%d" % (kind, m, n, k), worst)
    print("bnred", m, k, n, DT_IDS[dtype], worst)
    _fractions(worst)


# ---------------------------------------------------------------- planted faults
def _rejected(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e) or "assertion"
    return None


BNLOAD_FAULTS = [(f, r, kind) for f, r in (("msb", 0), ("drop_tile", 1), ("poison_row", 0)) for kind in ("exact", "gauss")] + \
                [("stats_unrounded", 1, "gauss"), ("res_unrounded", 2, "gauss")]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("fault, resmode, kind", BNLOAD_FAULTS)
def test_bnload_fault(fault, resmode, kind, dtype):
    """stats_unrounded and res_unrounded are planted in the Gaussian kind only: the exact inputs keep out and the branch output
    where 16-bit rounding changes nothing (else out^2 would leave the exactly summable 1/16 grid)."""
    m, k, n = M_RAGGED, 128, 128
    s = R.bnload_inputs(kind, dtype, CPU, m, k, n, resmode, 7)
    R.bnload_check(s, model_bnload(s, s.w), m, "honest", R.Worst())
    why = _rejected(lambda: R.bnload_check(s, model_bnload(s, s.w, fault), m, fault, R.Worst()))
    assert why is not None, "%s was accepted (%s)" % (fault, kind)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["exact", "gauss"])
@pytest.mark.parametrize("fault, wg", [("swap", False), ("swap", True), ("padded_m", False), ("padded_m", True), ("msb", False),
                                       ("msb", True), ("drop_tile", False), ("drop_tile", True), ("poison_row", False),
                                       ("poison_row", True), ("mean2_block", False)])
def test_bnbwd_fault(fault, wg, kind, dtype):
    m = M_RAGGED
    s = R.bnbwd_inputs(kind, dtype, CPU, m, True, True, 11)
    chains = {"bnred": m, "gw": m}
    R.bnbwd_check(s, model_bnbwd(s, wg), chains, "honest", R.Worst())
    why = _rejected(lambda: R.bnbwd_check(s, model_bnbwd(s, wg, fault), chains, fault, R.Worst()))
    assert why is not None, "%s was accepted (%s, wgrad form %s)" % (fault, kind, wg)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["exact", "gauss"])
@pytest.mark.parametrize("fault", ["msb", "drop_tile", "poison_row", "mean2_block"])
def test_bnred_fault(fault, kind, dtype):
    m, k, n = M_RAGGED, 64, 256
    s = R.bnred_inputs(kind, dtype, CPU, m, k, n, 13)
    R.bnred_check(s, model_bnred(s), m, "honest", R.Worst())
    why = _rejected(lambda: R.bnred_check(s, model_bnred(s, fault), m, fault, R.Worst()))
    assert why is not None, "%s was accepted (%s)" % (fault, kind)


def test_exact_preconditions_reject_unsummable_inputs():
    """check_exact guards the bit-exact bars: terms past the bound or off the grid must not reach a bit comparison."""
    s = R.bnred_inputs("exact", BF, CPU, M_RAGGED, 64, 128, 17)
    s.t2 = s.t2 * 0 + 0.125                                  # xhat2 leaves the 1/4 grid: dx xhat2 is off the 1/16 grid
    assert _rejected(lambda: R.bnred_check(s, model_bnred(s), M_RAGGED, "off grid", R.Worst())) is not None
