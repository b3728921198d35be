"""The kernels of csrc/fastpitch.hip against torch float64 / torch's own fp32 arithmetic.  GPU only.

Every kernel works on PACKED rows: sequence b owns rows cu[b] .. cu[b + 1] - 1 of a device int32 table; rows outside a row's own
sequence read as zero; lengths are clamped to [0, max_len] and rows to `total`.

dle_conv1d_packed_fwd.  Contract:  a = x < 0 ? round16(fl32(float(x) * slope)) : x;  acc = sum_k sum_c w[ko,k,c] a[r + k - (ksize-1)/2, c]
on the fp32 accumulator, zero outside the sequence;  y = round16(acc + bias (+ add1)).  Reference: torch float64 on the GPU, per
sequence, per tap a matrix product over a zero-padded shifted slice (no conv1d, nothing of this library).
  Tier 1, bit-exact: x, w, add1 = k / 4 with |k| <= 4 (tests/_exact_grid.py), bias a multiple of 1/64, slope 1 or 0: every term is a
  multiple of 1/16 of magnitude at most 1, at most 11 * 64 or 3 * 1536 = 4,608 of them, so the sum of magnitudes (addend and bias
  included) stays below B_MFMA = 2^18, every partial sum in any order is exact in fp32 and the output is the float64 value rounded
  ONCE.  The preconditions are asserted on the float64 side.
  Tier 2, random inputs (x, add1 ~ N(0,1), w ~ N(0, 1/(ksize C)), bias ~ N(0,1), rounded to storage first), per element, nothing
  skipped:  |got - ref| <= ulp16(ref) / 2 + (ksize C + 3) 2^-24 (sum|w a| + |bias| + |add1|): half a unit of the 16-bit format at the
  reference (the one rounding) plus the fp32 error of a (ksize C)-term sum and two additions.  Derived, not measured.
  Shapes -- the smallest at which each feature can fail.  The kernel gives a workgroup of 4 wavefronts TT = 64 rows of ONE sequence
  x CB = 128 output channels (a wavefront: 32 channels, two 32-row sub-tiles, the second skipped when the tile has <= 32 live rows);
  C is staged in chunks of 64 channels, 16 per MFMA step:
  * pack_k1 / pack_k3 / pack_k11 (C = Ko = 64): ONE pack of lengths (1, TT-1, TT, TT+1, 0, 2 TT + 2) = (1, 63, 64, 65, 0, 130):
    sequence boundaries fall inside what would be a tile of the packed rows, tile boundaries (64, 128) fall inside a sequence's
    halo on both sides, a zero-length sequence sits in the middle, the last tiles hold 1, 63, 1 and 2 rows (skipped second
    sub-tile), two idle wavefronts stage and meet the barriers (Ko = 64 of CB = 128).  The first and last (ksize-1)/2 rows of every
    sequence hold +-1 of a sign alternating with b: a tap that read a neighbour instead of zero would change every channel's sum;
  * ffn_up (384 -> 1536) and ffn_down (1536 -> 384) at the pack (5, 1): the network's two shapes: 12 / 3 channel blocks, 6 / 24 chunks;
  * tiny (8 -> 8, one sequence of 3 rows, max_len 1024: 15 of its 16 time tiles exit at once): half an MFMA step, 8 of 32 channels;
  * ko136 (24 -> 136, pack (70, 2)): a second channel block with 8 live channels (one partly filled wavefront, three idle); C = 24 is
    one and a half MFMA steps;  ko40 (24 -> 40, one sequence of 33 rows): the second wavefront partly filled;
  * c80_k3 / c80_k5 (80 -> 32, pack (40, 3)): C = one whole chunk + a 16-channel one: the operands of a PARTIAL chunk are loaded one
    chunk ahead, on both weight schedules of the kernel (all taps of a chunk held in registers for ksize <= 3, one tap ahead above).
  Variants: slope 1 / 0 (asserting that negative inputs occurred), add1 absent / present / aliasing y.
  A cu_seqlens whose last entry exceeds `total` is well-formed input for the clamp: the last sequence is cut at `total`, and the rows
  beyond it (the NaN tail of the output buffer) stay untouched.

dle_fp_relu_layernorm_fwd.  Exact: a row that is constant after the ReLU (all negative, or one positive value) gives round16(beta)
whatever gamma is (t - mean = 0 exactly: the sums of H <= 384 equal 11-bit values are exact in fp32); x and relu(x) give the same
bits.  Otherwise per element against float64:  |y - ref| <= ulp16(ref) / 2 + 2^-24 (|g| rstd ((H + 2) mean|t| + (H / 2 + 8) |t - mean|)
+ |beta| + |ref|): the mean of H terms and its division, the variance of H terms, its reciprocal square root, two products and a
sum, each at one fp32 unit, first order.  pred against float64 of the ROUNDED y the kernel wrote under (H + 1) 2^-24 (sum|fc_w y| +
|fc_b|); pred without y (want_y False) equals pred with y bit for bit.  H = 8, 64, 256, 384; rows = 1, and 2051 > 2048 = one trip
of the capped grid (512 workgroups x 4 rows).

dle_fp_embed, dle_fp_scalar_conv_add, dle_fp_expand, dle_fp_unpack_mel: bit for bit against torch written as the contract (fp32
additions and products in the stated order, one rounding).  Packs put sequence boundaries off the 16-row tile of these kernels.
expand: zero-repetition tokens at the start, in the middle and at the end of a sequence, a sequence whose tokens all have zero
repetitions, a repetition count of 75, frames across the 16-row tile.

dle_fp_durations.  Given durations: repetitions, token starts and the output table equal those of the torch expression of
model.py:47-55 evaluated on the HOST (fp32, IEEE division; torch's device kernel multiplies by a reciprocal instead): fractions of
exactly .5, pace 0.8 and 1.3, B = 1 and 5.  From log durations: dur_pred within 2 ulp32 (at exp(x)) of clamp(torch.exp(x) - 1, 0,
max) on the device -- that yardstick is torch's kernel, not ours -- with the clamp reached at 0 and at max_duration; reps equal to
float64's on inputs whose dur / pace stays >= 1e-3 from a rounding boundary (constructed so, asserted on the float64 side).

Outputs are views at the head of NaN-filled buffers whose tail must keep its bits.  Argument checks raise without a launch.
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
TT, CB, RT = 64, 128, 16

PACK = (1, TT - 1, TT, TT + 1, 0, 2 * TT + 2)
# name -> (lens, C, Ko, ksize, max_len or None for max(lens))
SHAPES = {
    "pack_k1": (PACK, 64, 64, 1, None),
    "pack_k3": (PACK, 64, 64, 3, None),
    "pack_k11": (PACK, 64, 64, 11, None),
    "ffn_up": ((5, 1), 384, 1536, 3, None),
    "ffn_down": ((5, 1), 1536, 384, 3, None),
    "tiny": ((3,), 8, 8, 3, 1024),
    "ko136": ((70, 2), 24, 136, 3, None),
    "ko40": ((33,), 24, 40, 3, None),
    "c80_k3": ((40, 3), 80, 32, 3, None),
    "c80_k5": ((40, 3), 80, 32, 5, None),
}
# name -> (slope, add1: 0 none / 1 present / 2 aliasing y)
VARIANTS = {"plain": (1.0, 0), "relu": (0.0, 0), "relu_add1": (0.0, 1), "inplace": (1.0, 2)}


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=DEV)


def act16(x, slope):
    return x if slope == 1.0 else torch.where(x < 0, (x.float() * slope).to(x.dtype), x)


def ref_packed_conv(a, w, lens):
    """(acc, mag) [total, Ko] float64: per sequence, per tap a product over a zero-padded shifted slice; mag = sum |w a|."""
    a, w = a.to(F64), w.to(F64)
    ko, ks, _ = w.shape
    halo = (ks - 1) // 2
    acc = torch.zeros((a.shape[0], ko), dtype=F64, device=a.device)
    mag = torch.zeros_like(acc)
    start = 0
    for n in lens:
        if n:
            ap = torch.nn.functional.pad(a[start:start + n], (0, 0, halo, halo))
            for k in range(ks):
                acc[start:start + n] += ap[k:k + n] @ w[:, k, :].t()
                mag[start:start + n] += ap[k:k + n].abs() @ w[:, k, :].abs().t()
        start += n
    return acc, mag


def run_conv(x, w, bias, lens, max_len, slope, add1, inplace=False, cu=None):
    o = Out((x.shape[0], w.shape[0]), x.dtype, DEV, fill=add1 if inplace else None)
    y = F.conv1d_packed_fwd(x, w, bias, cu_of(lens) if cu is None else cu, max_len or max(lens), slope=slope,
                            add1=o.t if inplace else add1, out=o.t)
    assert y.data_ptr() == o.t.data_ptr()
    torch.cuda.synchronize()
    return o.check("conv1d_packed_fwd")


@functools.lru_cache(maxsize=None)
def exact_inputs(name, dtype):
    lens, c, ko, ks, _ = SHAPES[name]
    total = sum(lens)
    x = grid((total, c), 11, dtype, DEV)
    h = (ks - 1) // 2
    if name.startswith("pack") and h:
        start = 0
        for b, n in enumerate(lens):
            sign = 1.0 if b % 2 == 0 else -1.0
            x[start:start + min(h, n)] = sign
            x[start + max(n - h, 0):start + n] = -sign
            start += n
    w = grid((ko, ks, c), 12, dtype, DEV)
    bias = torch.randint(-64, 65, (ko,), generator=gen(DEV, 13), device=DEV).float() / 64
    add1 = grid((total, ko), 14, dtype, DEV)
    return x, w, bias, add1


@functools.lru_cache(maxsize=None)
def exact_acc(name, dtype, slope):
    x, w, _, _ = exact_inputs(name, dtype)
    a = act16(x, slope)
    assert torch.equal(a.double() * 4, torch.round(a.double() * 4))
    acc, mag = ref_packed_conv(a, w, SHAPES[name][0])
    assert torch.equal(acc * 16, torch.round(acc * 16))
    assert float(mag.max()) + 2 < B_MFMA                                  # + |bias| + |add1|, each at most 1
    return acc


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv_exact_grid_bits(name, dtype, variant):
    slope, mode = VARIANTS[variant]
    lens, _, _, _, max_len = SHAPES[name]
    x, w, bias, add1 = exact_inputs(name, dtype)
    if slope != 1.0:
        assert bool((x < 0).any()), "no negative input for the ReLU"
    pre = exact_acc(name, dtype, slope) + bias.double()
    if mode:
        pre = pre + add1.double()
    assert torch.equal(pre * 64, torch.round(pre * 64)) and float(pre.abs().max()) < 2.0 ** 17
    got = run_conv(x, w, bias, lens, max_len, slope, add1 if mode else None, inplace=mode == 2)
    assert_same(bits(got), bits(pre.float().to(dtype)), "%s %s %s" % (name, dtype, variant))


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    lens, c, ko, ks, _ = SHAPES[name]
    g = gen(DEV, 21)
    total = sum(lens)
    x = torch.randn((total, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, ks, c), generator=g, device=DEV) * (ks * c) ** -0.5).to(dtype)
    bias = torch.randn((ko,), generator=g, device=DEV)
    add1 = torch.randn((total, ko), generator=g, device=DEV).to(dtype)
    return x, w, bias, add1


@pytest.mark.parametrize("slope", [1.0, 0.0], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv_random_inputs_per_element_bar(name, dtype, slope):
    lens, c, ko, ks, max_len = SHAPES[name]
    x, w, bias, add1 = random_case(name, dtype)
    assert bool((x < 0).any())
    acc, mag = ref_packed_conv(act16(x, slope), w, lens)
    ref = acc + bias.double() + add1.double()
    got = run_conv(x, w, bias, lens, max_len, slope, add1).double()
    bar = ulp16(ref, dtype) / 2 + (ks * c + 3) * U * (mag + bias.double().abs() + add1.double().abs())
    err = (got - ref).abs()
    worst = float((err / bar).max())
    print("%s %s slope %g: max err / bar %.3f" % (name, dtype, slope, worst))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bar).all()), "%s: %d of %d elements over the bar, worst ratio %.3f" % (name, int((err > bar).sum()), err.numel(), worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_table_beyond_total_is_clamped(dtype):
    """cu = (0, 5, 15) over 12 rows: the second sequence is cut to 7 rows; nothing behind row 11 is written."""
    c, ko, ks = 16, 16, 3
    x = grid((12, c), 31, dtype, DEV)
    w = grid((ko, ks, c), 32, dtype, DEV)
    bias = torch.zeros(ko, device=DEV)
    acc, _ = ref_packed_conv(x, w, (5, 7))
    got = run_conv(x, w, bias, (5, 10), 10, 1.0, None, cu=torch.tensor([0, 5, 15], dtype=torch.int32, device=DEV))
    assert_same(bits(got), bits(acc.float().to(dtype)), "clamped table %s" % dtype)


def test_conv_argument_checks_raise_without_a_launch():
    z = lambda *s, dt=BF: torch.zeros(s, dtype=dt, device=DEV)
    x, w, bias, cu = z(16, 16), z(8, 3, 16), torch.zeros(8, device=DEV), cu_of((16,))
    F.conv1d_packed_fwd(x, w, bias, cu, 16)                              # the baseline call is inside the envelope
    bad = [
        lambda: F.conv1d_packed_fwd(z(16, 12), z(8, 3, 12), bias, cu, 16),                   # C = 12
        lambda: F.conv1d_packed_fwd(x, z(8, 4, 16), bias, cu, 16),                           # even ksize
        lambda: F.conv1d_packed_fwd(x, z(8, 13, 16), bias, cu, 16),                          # ksize 13
        lambda: F.conv1d_packed_fwd(x.float(), w.float(), bias, cu, 16),                     # fp32
        lambda: F.conv1d_packed_fwd(x, w, bias, cu, 1025),                                   # max_len above the envelope
        lambda: F.conv1d_packed_fwd(x, w, bias, cu, 0),
        lambda: F.conv1d_packed_fwd(x, w, bias, cu.long(), 16),                              # an int64 table
        lambda: F.conv1d_packed_fwd(x, w, torch.zeros(9, device=DEV)[1:], cu, 16),           # a misaligned bias
        lambda: F.conv1d_packed_fwd(x, z(16, 3, 16), torch.zeros(16, device=DEV), cu, 16, out=x),    # y over x
        lambda: F.conv1d_packed_fwd(x, w, bias, cu, 16, add1=z(16, 16)),                     # add1 of the wrong width
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()


# ---- relu + LayerNorm (+ fc) -----------------------------------------------------------------------------------------------------
LN_CASES = [(8, 1), (8, 2051), (64, 5), (256, 2051), (384, 33)]
EPS = 1e-5


def ln_params(h, n_pred, seed):
    g = gen(DEV, seed)
    gamma = 1.0 + 0.5 * torch.randn(h, generator=g, device=DEV)
    beta = torch.randn(h, generator=g, device=DEV)
    fc_w = torch.randn((n_pred, h), generator=g, device=DEV) * h ** -0.5
    fc_b = torch.randn(n_pred, generator=g, device=DEV)
    return gamma, beta, fc_w, fc_b


def run_ln(x, gamma, beta, fc_w=None, fc_b=None, want_y=True):
    rows, h = x.shape
    oy = Out((rows, h), x.dtype, DEV) if want_y else None
    op = Out((rows, fc_w.shape[0]), torch.float32, DEV) if fc_w is not None else None
    F.fp_relu_layernorm_fwd(x, gamma, beta, eps=EPS, fc_w=fc_w, fc_b=fc_b, want_y=want_y, out=oy.t if oy else None,
                            pred_out=op.t if op else None)
    torch.cuda.synchronize()
    return (oy.check("relu_layernorm y") if oy else None), (op.check("relu_layernorm pred") if op else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [8, 64, 256, 384])
def test_relu_layernorm_constant_rows_give_beta_and_relu_is_a_mask(h, dtype):
    gamma, beta, _, _ = ln_params(h, 1, 41)
    x = torch.randn((6, h), generator=gen(DEV, 42), device=DEV).to(dtype)
    x[0] = -x[0].abs() - 1                                                # all negative: t = 0
    x[1] = 0.75
    x[2] = 3.0
    x[3] = torch.where(torch.arange(h, device=DEV) % 2 == 0, -1.0, -0.0).to(dtype)
    y, _ = run_ln(x, gamma, beta)
    want = beta.to(dtype)
    for r in range(4):
        assert_same(bits(y[r]), bits(want), "constant row %d H %d %s" % (r, h, dtype))
    assert bool((x[4:] < 0).any())
    y2, _ = run_ln(torch.relu(x), gamma, beta)
    assert_same(bits(y), bits(y2), "relu(x) and x H %d %s" % (h, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "H%d_R%d" % c)
def test_relu_layernorm_per_element_bar_and_pred(case, dtype):
    h, rows = case
    n_pred = 1 + (h // 8) % 4 if h != 384 else 4                          # 2, 1, 1, 4: every count appears somewhere
    gamma, beta, fc_w, fc_b = ln_params(h, n_pred, 51)
    x = (torch.randn((rows, h), generator=gen(DEV, 52), device=DEV) * 2).to(dtype)
    assert bool((x < 0).any())
    y, pred = run_ln(x, gamma, beta, fc_w, fc_b)
    t = torch.relu(x.double())
    mu = t.mean(1, keepdim=True)
    d = t - mu
    rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
    g, b = gamma.double(), beta.double()
    ref = d * rstd * g + b
    bar = ulp16(ref, dtype) / 2 + U * (g.abs() * rstd * ((h + 2) * t.abs().mean(1, keepdim=True) + (h / 2 + 8) * d.abs()) + b.abs() + ref.abs())
    err = (y.double() - ref).abs()
    worst = float((err / bar).max())
    pref = y.double() @ fc_w.double().t() + fc_b.double()
    pbar = (h + 1) * U * (y.double().abs() @ fc_w.double().abs().t() + fc_b.double().abs())
    perr = (pred.double() - pref).abs()
    pworst = float((perr / pbar).max())
    print("relu_ln H %d rows %d %s: y max err / bar %.3f, pred max err / bar %.3f" % (h, rows, dtype, worst, pworst))
    assert tuple(pred.shape) == (rows, n_pred)
    assert bool((err <= bar).all()), "%d of %d y elements over the bar, worst %.3f" % (int((err > bar).sum()), err.numel(), worst)
    assert bool((perr <= pbar).all()), "%d of %d pred elements over the bar, worst %.3f" % (int((perr > pbar).sum()), perr.numel(), pworst)
    _, pred_only = run_ln(x, gamma, beta, fc_w, fc_b, want_y=False)
    assert_same(bits(pred_only), bits(pred), "pred without y")


def test_relu_layernorm_argument_checks():
    x = torch.zeros((4, 16), dtype=BF, device=DEV)
    g, b = torch.ones(16, device=DEV), torch.zeros(16, device=DEV)
    F.fp_relu_layernorm_fwd(x, g, b)
    bad = [
        lambda: F.fp_relu_layernorm_fwd(x.float(), g, b),
        lambda: F.fp_relu_layernorm_fwd(torch.zeros((4, 1032), dtype=BF, device=DEV), torch.ones(1032, device=DEV), torch.zeros(1032, device=DEV)),
        lambda: F.fp_relu_layernorm_fwd(torch.zeros((4, 12), dtype=BF, device=DEV), torch.ones(12, device=DEV), torch.zeros(12, device=DEV)),
        lambda: F.fp_relu_layernorm_fwd(x, g, b, fc_w=torch.zeros((5, 16), device=DEV), fc_b=torch.zeros(5, device=DEV)),
        lambda: F.fp_relu_layernorm_fwd(x, g, b, fc_w=torch.zeros((1, 16), device=DEV)),
        lambda: F.fp_relu_layernorm_fwd(x, g, b, want_y=False),
        lambda: F.fp_relu_layernorm_fwd(x, g[:8], b),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()


# ---- the row kernels: bit for bit against torch's fp32 arithmetic ----------------------------------------------------------------
ROW_PACK = (1, RT + 1, 0, RT, 2 * RT + 1)


def positions(lens):
    return torch.cat([torch.arange(n, device=DEV) for n in lens])


@pytest.mark.parametrize("with_spk", [False, True], ids=["nospk", "spk"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [24, 128])
def test_embed_bits(d, dtype, with_spk):
    g = gen(DEV, 61)
    total, n_sym = sum(ROW_PACK), 37
    ids = torch.randint(0, n_sym, (total,), generator=g, device=DEV)
    word = torch.randn((n_sym, d), generator=g, device=DEV)
    pos = torch.randn((max(ROW_PACK) + 3, d), generator=g, device=DEV)
    spk = torch.randn(d, generator=g, device=DEV) if with_spk else None
    want = word[ids] + pos[positions(ROW_PACK)]
    if with_spk:
        want = want + spk
    o = Out((total, d), dtype, DEV)
    F.fp_embed(ids, word, pos, cu_of(ROW_PACK), max(ROW_PACK), dtype, spk=spk, out=o.t)
    torch.cuda.synchronize()
    assert_same(bits(o.check("fp_embed")), bits(want.to(dtype)), "embed D %d %s" % (d, dtype))
    with pytest.raises(ValueError):                                      # the positional table is shorter than max_len
        F.fp_embed(ids, word, pos[:8].contiguous(), cu_of(ROW_PACK), max(ROW_PACK), dtype)
    with pytest.raises(ValueError):
        F.fp_embed(ids.int(), word, pos, cu_of(ROW_PACK), max(ROW_PACK), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ks", [1, 3, 5])
def test_scalar_conv_add_bits(ks, dtype):
    g = gen(DEV, 71)
    total, d = sum(ROW_PACK), 40
    enc = torch.randn((total, d), generator=g, device=DEV).to(dtype)
    v = torch.randn(total, generator=g, device=DEV)
    w = torch.randn((d, ks), generator=g, device=DEV)
    bias = torch.randn(d, generator=g, device=DEV)
    s = bias[None, :].expand(total, d).clone()
    halo = (ks - 1) // 2
    start = 0
    for n in ROW_PACK:
        if n:
            vp = torch.nn.functional.pad(v[start:start + n], (halo, halo))
            for k in range(ks):
                prod = w[:, k][None, :] * vp[k:k + n][:, None]            # one rounding
                s[start:start + n] = s[start:start + n] + prod              # a second one: no fused multiply-add
        start += n
    want = (enc.float() + s).to(dtype)
    o = Out((total, d), dtype, DEV, fill=enc)
    F.fp_scalar_conv_add_(o.t, v, w, bias, cu_of(ROW_PACK), max(ROW_PACK))
    torch.cuda.synchronize()
    assert_same(bits(o.check("fp_scalar_conv_add")), bits(want), "scalar conv ks %d %s" % (ks, dtype))
    with pytest.raises(ValueError):
        F.fp_scalar_conv_add_(o.t, v, torch.zeros((d, 4), device=DEV), bias, cu_of(ROW_PACK), max(ROW_PACK))


EXPAND_REPS = ([0, 0, 3, 0, 75, 1, 0], [0, 0, 0], [20, 20], [1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_expand_bits(dtype):
    g = gen(DEV, 81)
    d = 72
    in_lens = [len(r) for r in EXPAND_REPS]
    out_lens = [sum(r) for r in EXPAND_REPS]
    assert out_lens == [79, 0, 40, 1]
    reps = torch.tensor(sum(EXPAND_REPS, []), dtype=torch.int32, device=DEV)
    tok_start = torch.tensor(sum(([sum(r[:i]) for i in range(len(r))] for r in EXPAND_REPS), []), dtype=torch.int32, device=DEV)
    total_in, total_out = sum(in_lens), sum(out_lens)
    enc = torch.randn((total_in, d), generator=g, device=DEV).to(dtype)
    pos = torch.randn((80, d), generator=g, device=DEV)
    src = torch.repeat_interleave(torch.arange(total_in, device=DEV), reps.long())
    want = (enc[src].float() + pos[positions(out_lens)]).to(dtype)
    o = Out((total_out, d), dtype, DEV)
    F.fp_expand(enc, pos, reps, tok_start, cu_of(in_lens), cu_of(out_lens), max(in_lens), max(out_lens), total_out, out=o.t)
    torch.cuda.synchronize()
    assert_same(bits(o.check("fp_expand")), bits(want), "expand %s" % dtype)
    with pytest.raises(ValueError):                                      # a positional table shorter than max_out
        F.fp_expand(enc, pos[:40].contiguous(), reps, tok_start, cu_of(in_lens), cu_of(out_lens), max(in_lens), max(out_lens), total_out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_mel", [8, 80])
def test_unpack_mel_bits(n_mel, dtype):
    lens, t_pad = (5, 0, 70, 64), 70
    g = gen(DEV, 91)
    x = torch.randn((sum(lens), n_mel), generator=g, device=DEV).to(dtype)
    bias = torch.randn(n_mel, generator=g, device=DEV)
    want = bias[None, :, None].expand(len(lens), n_mel, t_pad).clone()
    start = 0
    for b, n in enumerate(lens):
        want[b, :, :n] = x[start:start + n].float().t()
        start += n
    o = Out((len(lens), n_mel, t_pad), torch.float32, DEV)
    F.fp_unpack_mel(x, bias, cu_of(lens), t_pad, out=o.t)
    torch.cuda.synchronize()
    assert_same(bits(o.check("fp_unpack_mel")), bits(want), "unpack_mel %d %s" % (n_mel, dtype))
    with pytest.raises(ValueError):
        F.fp_unpack_mel(x, bias, cu_of(lens), 1025)


# ---- durations -------------------------------------------------------------------------------------------------------------------
def host_regulate(dur, pace, lens):
    """model.py:47-55 on the host in fp32: reps, per-sequence exclusive cumsum, the output table."""
    reps = ((dur.cpu().float() / pace) + 0.5).long()
    starts, cu, at = [], [0], 0
    for n in lens:
        r = reps[at:at + n]
        starts.append(torch.cumsum(r, 0) - r)
        cu.append(cu[-1] + int(r.sum()))
        at += n
    return reps.int(), torch.cat(starts).int(), torch.tensor(cu, dtype=torch.int32)


@pytest.mark.parametrize("lens", [(7,), (1, 12, 3, 9, 20)], ids=["B1", "B5"])
@pytest.mark.parametrize("pace", [1.0, 0.8, 1.3])
def test_durations_given_bits(pace, lens):
    g = gen(DEV, 101)
    total = sum(lens)
    dur = torch.rand(total, generator=g, device=DEV) * 12
    dur[::3] = torch.randint(0, 9, ((total + 2) // 3,), generator=g, device=DEV).float() + 0.5     # fractions of exactly .5
    dur[1::5] = torch.randint(0, 76, ((total + 3) // 5,), generator=g, device=DEV).float()         # integers, 0 and 75 among the range
    dur[0] = 0.0
    dur[-1] = 75.0
    want = host_regulate(dur, pace, lens)
    _, reps, tok_start, cu_out = F.fp_durations(dur, cu_of(lens), max(lens), pace=pace, from_log=False, max_out=1 << 30)
    torch.cuda.synchronize()
    for got, ref, what in zip((reps, tok_start, cu_out), want, ("reps", "tok_start", "cu_out")):
        assert_same(got.cpu(), ref, "%s pace %g" % (what, pace))


@pytest.mark.parametrize("pace", [1.0, 0.8])
def test_durations_from_log(pace):
    lens = (1, 12, 3, 9, 20)
    total = sum(lens)
    g = gen(DEV, 111)
    k = torch.randint(0, 12, (total,), generator=g, device=DEV).double()
    frac = torch.rand(total, generator=g, device=DEV).double() * 0.496 + 0.002
    frac = torch.where(torch.rand(total, generator=g, device=DEV) < 0.5, frac, frac + 0.5)
    q = k + frac                                                          # dur / pace: 2e-3 from every k + 0.5 at least
    x = torch.log(q * pace + 1).float()
    x[0], x[5], x[7] = -3.0, 9.0, 0.0                                     # the clamp at 0 (exp(-3) - 1 < 0) and at max_duration; dur = 0
    dur64 = torch.clamp(torch.exp(x.double()) - 1, 0, 75.0)
    q64 = dur64 / float(torch.tensor(pace, dtype=torch.float32))
    assert float(((q64 - torch.floor(q64)) - 0.5).abs().min()) >= 1e-3
    dur, reps, tok_start, cu_out = F.fp_durations(x, cu_of(lens), max(lens), pace=pace, max_duration=75, max_out=1 << 30)
    torch.cuda.synchronize()
    e = torch.exp(x)                                                      # torch's device kernel: the yardstick
    ref = torch.clamp(e - 1, 0, 75.0)
    _, ex = torch.frexp(e.double())
    bar = 2 * torch.pow(2.0, (ex - 1).double() - 23)
    err = (dur.double() - ref.double()).abs()
    print("durations from log, pace %g: max err %.3f ulp32 of exp(x)" % (pace, float((err / (bar / 2)).max())))
    assert bool((err <= bar).all())
    assert float(dur[0]) == 0.0 and float(dur[5]) == 75.0 and float(dur[7]) == 0.0
    want = torch.floor(q64 + 0.5).int().cpu()
    assert_same(reps.cpu(), want, "reps from log durations")
    _, starts, cu = host_regulate(want.float(), 1.0, lens)
    assert_same(tok_start.cpu(), starts, "tok_start")
    assert_same(cu_out.cpu(), cu, "cu_out")


def test_durations_argument_checks():
    x = torch.zeros(4, device=DEV)
    cu = cu_of((4,))
    bad = [
        lambda: F.fp_durations(x, cu, 4, pace=0.0),
        lambda: F.fp_durations(x.half(), cu, 4),
        lambda: F.fp_durations(x, cu.long(), 4),
        lambda: F.fp_durations(x, cu, 2000),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()
