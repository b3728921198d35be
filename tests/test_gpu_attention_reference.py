"""The fused attention kernels of csrc/attention.hip (attn_fwd, attn_bwd, attn_fwd_long, attn_bwd_dq_long, attn_bwd_dkv_long) against
the float64 statement, exact inputs and derived bars of tests/_attention_reference.py.  GPU only; tests/test_gpu_attention.py keeps
the whole-tensor checks, this file holds every ELEMENT to a bar.  Every output (ctx, dqkv, stats, keep mask, colsum_partial) is a
view at the head of a NaN / 0xFF-filled buffer (tests/_exact_grid.Out) through the C ABI: the tails must keep their bits and every
element the contract promises must be written.

Shapes (S, B, heads): (128,1,1) (128,3,3) (256,2,3) (384,2,2) (640,1,3) (1024,1,2): one kernel each way and the streaming
kernels with 2, 3, 5 and 8 key blocks, 1 / 2 / 3 heads, B = 1; (1024,2,16) for the selector only (chunk index up to 2^22).

EXACT CASES (bit for bit, +0 = -0; every element, nothing sampled).  All inputs are k / 4 grids.
* Selector.  Rows of Q and K are two-hot codes 32 (e_a + e_b) and scale = 1/8, so scores are 0, 128 or 256: every query q has one
  key pi(q) at 256 and nothing else above 128 (or 128 - 10000 under the mask).  fp32 exp(-128) = 0 (the gap at which this holds
  is 104: exp(-104) < 2^-150), so P is exactly 0 / 1 -- also through the online max / sum, whose rescale factor is then 0 or 1 --
  inv = 1, mx = 256, ctx[q] = inv_keep keep V[pi(q)], dP - delta = 0 at the one key with P = 1, hence dq = dk = 0 and dv[k] = the
  sum of inv_keep dO[q] over the kept q with pi(q) = k.  pi is 2-to-1, leaves keys unchosen, picks the first, a middle and the last
  key block inside every workgroup, crosses blocks both ways and lands on all 8 positions of a 16-byte chunk.  p = 0 and p = 0.5
  (thr = 32768, inv_keep = 2: no rounding), keep mask = the Philox oracle's = the bytes the forward kernel returns.
* Uniform.  Q = 0 (or K = 0): all scores are 0, the mask is -10000 on all but n_valid scattered keys (1, 32, 64, 128, S; one
  sequence entirely -10000): P = 1 / n_valid exactly on the valid keys, 0 elsewhere, ctx an exact mean.  dO lives on 32 dimensions
  on which V sums to 0 over the valid keys: delta = 0, |dP| < 16, so dS = P dP has 8 significant bits and dq (dk when K = 0) and
  dv are exact sums; rows of dk / dv at padded keys are exactly 0.  p = 0.5: forward exact, backward under the bars below.
  One more forward case has n_valid = 3 (fp16) / a small n that is no power of two and p = 0.1: dropout(P) is then the 16-bit
  rounding of fp32(1 / n) x fp32(inv_keep), which differs from rounding 1 / n first.
* colsum_partial equals the column sums of the STORED dqkv exactly (the stored values are on a grid: any order gives the same).

GENERIC CASES (seeded N(0, sigma) in fp16 / bf16, sigma 0.8 and 3 -- scores reach tens, the online rescale works --, scattered
mask, p = 0 and 0.1 with the kernel's own keep mask checked against the oracle first).  u = 2^-24, m = 10 / 7 mantissa bits.
The kernels keep scores, probabilities and every sum in fp32 and round exactly two kinds of things to 16 bits: the operands
dropout(P) and dS of the second contractions, and the stored outputs.  For an output x = sum_k a_k b_k with a the rounded operand:
    |got - ref| <= sum_k rnd(a_k) |b_k|      one rounding of the operand: rnd(a) = max(2^-(m+1) |a|, half the subnormal spacing)
                 + n u M                     fp32 accumulation, M = sum_k |a_k| |b_k|, n = S + log2 S (length + reduction levels)
                 + sum_k e_P |a_k| |b_k|     the fp32 probability inside a: e_P = (3 (|v| + |max|) + 20) u  (test_gpu_bert_rowops)
                 + 1 ulp16(ref) + 2 u |ref|  the stored rounding (1 ulp: the fp32 value may sit across a tie), torch's conversion
with M = |Pd| |V| (ctx), |dS| |K| (dq), |dS|^T |Q| (dk), |Pd|^T |dO| (dv).  dq and dk add the cancellation in dS = P (dP - delta)
scale, carried through the same product: [u (|dP| + |delta|) + err(dP) + err(delta)] P scale with err(dP) = 5 u inv_keep |dO| |V|
(four matrix-instruction accumulations and the dropout product) and err(delta) = sum_k P (e_P |dP| + err(dP)) + (S / 2 + 2) u
sum_k P |dP| (delta is an fp32 chain over the lane's S / 2 keys).  Row statistics: max within 6 u (sum |q| |k| scale + |mask|) at
the keys within 1 of the maximum (four accumulations, the scale, the mask); 1 / sum within sum_k e_P P + (70 nblk + (nblk - 1)
(6 A + 20)) u relative (the sum chain and the online rescale factors; A = the largest contributing |score|).
Three of these terms are not in the short form "(2^-(m+1) + n u) M + e_P M + ulp + 2 u |ref| + u (|dP| + |delta|) P scale" and
"max within 2 u (1 + |max|)": the subnormal half-spacing of an fp16 operand (P below 2^-14 is rounded with an ABSOLUTE error
2^-25; at S >= 128 and sigma = 3 most probabilities are that small), err(dP) + err(delta), and the accumulation of the score.
An fp32 evaluation on the CPU with exact 16-product groups (tests/test_attention_reference_host.py) leaves the short form by
up to 11.7 x (ctx) / 10.5 x (dq) / 5.7 x (dk) / 2.4 x (dv) / 1.3 x (max) and stays below 0.93 x with the three terms; the short
form's ratios are recorded beside the others ("lit_"), the bars asserted are the full ones.
Per (sequence, head, 128-row block) the relative L2 error is at most 2^-(m+1) for ctx and 2 x 2^-(m+1) for dq / dk / dv (every
element's rounding is at most that, relative; the operand roundings are independent and average down): a prediction of the model.

Worst |error| / bar on the MI355X over the six shapes and p = 0 / 0.1 (a record; the pass condition is <= 1; test_zz_report_ratios
prints them with -s).  "L2": the per-block relative L2 over its bar; "short": the per-element ratio under the short form above.
                 ctx    dq     dk     dv   | L2 ctx   dq     dk     dv   | max    1/sum  colsum | short ctx    dq     dk     dv    max
  fp16 sigma 0.8 0.330  0.402  0.341  0.283 | 0.626  0.312  0.311  0.320 | 0.265  0.070  0.039  |       0.330  0.409  0.345  0.283  1.004
  fp16 sigma 3   0.747  0.749  0.704  0.772 | 0.679  0.350  0.334  0.340 | 0.294  0.132  0.027  |      11.689 10.502  5.700  2.447  1.518
  bf16 sigma 0.8 0.355  0.406  0.325  0.288 | 0.629  0.310  0.310  0.318 | 0.282  0.061  0.032  |       0.355  0.406  0.325  0.288  1.113
  bf16 sigma 3   0.836  0.903  0.771  0.922 | 0.656  0.348  0.343  0.335 | 0.249  0.143  0.031  |       0.836  2.555  0.791  0.922  1.329
The CPU model's largest ratios are the same to three digits for ctx / dq / dk / dv (0.836 / 0.903 / 0.771 / 0.922: the stored bits
agree at those elements), 0.257 for the max and 0.153 for 1 / sum.  Every exact case passed bit for bit on the first run: no
kernel change was needed.  The short form fails on the hardware as it does on the CPU (fp16 operands below 2^-14, the bf16 dq
cancellation, the row max), which is what the three added terms account for.
"""
import pytest
import torch

from tests import _attention_reference as A
from tests import _exact_grid as G

pytestmark = pytest.mark.gpu

SEED, OFF = 0x1234567887654321, (1 << 34) + 9
RATIOS = {}


def _C():
    from deeplearningexamples_amd import _cabi as C
    return C


def _run(cuda, qkv, dctx, mask_add, b, s, nh, scale, p, seed=SEED, off=OFF, base=None, keep_read=False, bwd=True, want_mask=True):
    """dle_attention_fwd (+ dle_attention_bwd / _bwd_keep) through the C ABI into guarded buffers.  -> CPU tensors: ctx, dq, dk, dv
    [b, nh, s, 64], mx, inv [b, nh, s], mbytes (or None), dqkv [T, 3H] and colsum [b s / 128, 3H] as stored."""
    C = _C()
    T, H, dt = b * s, nh * A.D, qkv.dtype
    qkv_d, dctx_d = qkv.to(cuda).contiguous(), dctx.to(cuda).contiguous()
    mask_d = None if mask_add is None else mask_add.to(cuda).float().contiguous()
    base_d = None if base is None else torch.tensor([base], dtype=torch.int64, device=cuda)
    sw = int(C.lib().dle_attention_stats_floats(s))
    ctx, stats = G.Out((T, H), dt, cuda), G.Out((b * nh, s, sw), torch.float32, cuda)
    mb = G.Out((b * nh * s * s // 8,), torch.uint8, cuda) if (p > 0 and want_mask) else None
    C.call("dle_attention_fwd", C.ptr(qkv_d), C.ptr(mask_d), C.ptr(ctx.t), C.ptr(stats.t), C.ptr(mb.t) if mb else 0, b, s, nh, A.D,
           float(scale), float(p), seed, off, C.ptr(base_d), C.dt(qkv_d), C.stream())
    torch.cuda.synchronize()
    out = dict(ctx=A.heads(ctx.check("attention_fwd ctx").cpu(), b, s, nh))
    st = stats.check("attention_fwd stats").cpu()
    assert not bool(torch.isnan(out["ctx"].float()).any()), "ctx: an element was not written"
    assert not bool(torch.isnan(st[..., 0:2]).any()), "stats: a (max, 1 / sum) pair was not written"
    if sw == 4:
        assert bool(torch.isnan(st[..., 2:4]).all()), "attention_fwd wrote the backward pass's words of a statistics row"
    out["mx"], out["inv"] = st[..., 0].reshape(b, nh, s), st[..., 1].reshape(b, nh, s)
    out["mbytes"] = mb.check("attention_fwd keep mask").cpu() if mb else None
    if not bwd:
        return out
    dqkv, cs = G.Out((T, 3 * H), dt, cuda), G.Out((b * (s // A.BLK), 3 * H), torch.float32, cuda)
    tail = [C.ptr(dqkv.t), C.ptr(cs.t), b, s, nh, A.D, float(scale), float(p), seed, off, C.ptr(base_d), C.dt(qkv_d), C.stream()]
    if keep_read:
        C.call("dle_attention_bwd_keep", C.ptr(qkv_d), C.ptr(dctx_d), C.ptr(mask_d), C.ptr(stats.t), C.ptr(mb.t), *tail)
    else:
        C.call("dle_attention_bwd", C.ptr(qkv_d), C.ptr(dctx_d), C.ptr(mask_d), C.ptr(stats.t), *tail)
    torch.cuda.synchronize()
    out["dqkv"], out["colsum"] = dqkv.check("attention_bwd dqkv").cpu(), cs.check("attention_bwd colsum_partial").cpu()
    st2 = stats.check("attention_bwd stats").cpu()
    assert torch.equal(st2[..., 0:2], st[..., 0:2]), "attention_bwd changed (max, 1 / sum)"
    if sw == 4:
        assert bool(torch.isnan(st2[..., 3]).all()) and not bool(torch.isnan(st2[..., 2]).any())
    if mb:
        assert torch.equal(mb.check("attention_bwd keep mask").cpu(), out["mbytes"])
    assert not bool(torch.isnan(out["dqkv"].float()).any()) and not bool(torch.isnan(out["colsum"]).any()), "an element was not written"
    for i, nm in enumerate(("dq", "dk", "dv")):
        out[nm] = A.heads(out["dqkv"][:, i * H:(i + 1) * H], b, s, nh)
    return out


def _keep_checked(out, b, s, nh, p, seed=SEED, off=OFF):
    """The Philox oracle's keep mask, after the bytes the forward kernel returned are checked against it."""
    if p == 0:
        return None
    keep = A.oracle_keep(b, nh, s, p, seed, off)
    G.assert_same(out["mbytes"], A.pack_keep(keep), "keep mask bytes against the Philox oracle")
    return keep


def _colsum_exact(out, what):
    A.check_colsum(out["dqkv"].double(), what)
    G.assert_same(out["colsum"].double(), A.colsum_ref(out["dqkv"]), what + " colsum_partial")


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("shape", A.SHAPES + [A.BIG], ids=A.shape_id)
def test_selector_exact(cuda, shape, dtype):
    """P exactly 0 / 1 through every kernel: gathers, the key permutation of the transpose reads, the online max / sum, the Philox
    chunk index of three kernels and the forward / backward agreement on P, bit for bit.  (128,1,1) runs without a mask (NULL)."""
    s, b, nh = shape
    case = A.Selector(s, b, nh, dtype, with_mask=b > 1)
    for p in (0.0, 0.5):
        out = _run(cuda, case.qkv, case.dctx, case.mask_add, b, s, nh, case.scale, p)
        keep = _keep_checked(out, b, s, nh, p)
        A.check_selector(out, case, keep, A.inv_keep(p), "selector p %g" % p)
        _colsum_exact(out, "selector p %g" % p)


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("mirror", [False, True], ids=["q0", "k0"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_uniform_exact(cuda, shape, mirror, dtype):
    """P = 1 / n_valid on scattered valid keys: the float4 mask reads, exact means, exact dq / dk / dv, zero rows at padded keys,
    a fully padded sequence; p = 0.5: exact forward, backward under the derived bars."""
    s, b, nh = shape
    for plan in A.PLANS[shape]:
        case = A.Uniform(s, b, nh, dtype, plan, mirror)
        what = "uniform %s" % plan
        out = _run(cuda, case.qkv, case.dctx, case.mask_add, b, s, nh, case.scale, 0.0)
        A.check_uniform_fwd(out, case, None, 1.0, what)
        A.check_uniform_bwd(out, case, what)
        _colsum_exact(out, what)
        out = _run(cuda, case.qkv, case.dctx, case.mask_add, b, s, nh, case.scale, 0.5)
        keep = _keep_checked(out, b, s, nh, 0.5)
        A.check_uniform_fwd(out, case, keep, 2.0, what + " p 0.5")
        r = A.reference(case.qkv, case.dctx, case.mask_add, keep, b, s, nh, case.scale, 2.0)
        A.check_generic({k: out[k] for k in ("dq", "dk", "dv")}, r, dtype, what + " p 0.5")


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_uniform_rounding_after_scale(cuda, dtype):
    """P = 1 / n, n no power of two, p = 0.1: the stored dropout(P) is ONE rounding of fp32(1 / n) fp32(inv_keep) (rounding 1 / n
    first gives other bits), everything around it exact: ctx and the statistics bit for bit."""
    s, b, nh, p = 128, 1, 1, 0.1
    ik = A.inv_keep(p)
    case = A.Uniform(s, b, nh, dtype, [A.odd_n(dtype, ik)], pair=False)
    out = _run(cuda, case.qkv, case.dctx, case.mask_add, b, s, nh, case.scale, p, bwd=False)
    A.check_uniform_fwd(out, case, _keep_checked(out, b, s, nh, p), ik, "uniform n %s p 0.1" % case.plan)


# ------------------------------------------------------------------------------------------------ generic cases
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("sigma", [0.8, 3.0])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_generic_bars(cuda, shape, sigma, p, dtype):
    s, b, nh = shape
    qkv, dctx, mask_add = A.generic_inputs(s, b, nh, dtype, sigma)
    out = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p)
    keep = _keep_checked(out, b, s, nh, p)
    r = A.reference(qkv, dctx, mask_add, keep, b, s, nh, 0.125, A.inv_keep(p))
    sink = RATIOS.setdefault((A.name(dtype), sigma), {})
    A.check_generic({k: out[k] for k in ("ctx", "dq", "dk", "dv", "mx", "inv")}, r, dtype, "generic", sink)
    # column sums of the stored gradient: 32 rows per lane, then the 4 waves: an fp32 chain of 34
    terms = out["dqkv"].double().abs().view(-1, A.BLK, out["dqkv"].shape[-1]).sum(1)
    rt, i = A.ratio(out["colsum"], A.colsum_ref(out["dqkv"]), 34 * A.U * terms + 2.0 ** -140)
    sink["colsum"] = max(sink.get("colsum", 0.0), rt)
    assert rt <= 1.0, "colsum_partial: |error| / bar = %.3f at %d" % (rt, i)


# ------------------------------------------------------------------------------------------------ contracts
@pytest.mark.parametrize("s", [128, 256])
def test_offset_base(cuda, s):
    """A device word b0 with offset = o gives the bits of offset = o + b0 (a sum that carries across bit 32): the forward kernel and
    both backward forms at S = 128 (re-drawn and read keep mask), the three streaming kernels at S = 256."""
    b, nh, p, dtype = 2, 3, 0.1, torch.bfloat16
    qkv, dctx, mask_add = A.generic_inputs(s, b, nh, dtype, 0.8)
    o, b0 = 0xFFFFFFF0, 0x25
    want = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p, off=o + b0)
    _keep_checked(want, b, s, nh, p, off=o + b0)
    other = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p, off=o, bwd=False)
    assert not torch.equal(other["mbytes"], want["mbytes"])
    for keep_read in (False, True):
        got = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p, off=o, base=b0, keep_read=keep_read)
        for nm in ("mbytes", "ctx", "dqkv", "colsum", "mx", "inv"):
            assert torch.equal(G.bits(got[nm].contiguous()), G.bits(want[nm].contiguous())), (nm, keep_read)


@pytest.mark.parametrize("s", [128, 256])
def test_keep_mask_read_or_ignored(cuda, s):
    """keep_mask= in the backward pass: read at S = 128, ignored (the mask is re-drawn) at S = 256 -- where a WRONG mask must not
    change a bit; the same bits as the re-drawn path either way."""
    b, nh, p, dtype = 2, 3, 0.1, torch.float16
    qkv, dctx, mask_add = A.generic_inputs(s, b, nh, dtype, 0.8)
    want = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p)
    got = _run(cuda, qkv, dctx, mask_add, b, s, nh, 0.125, p, keep_read=True)
    assert torch.equal(G.bits(got["dqkv"]), G.bits(want["dqkv"])) and torch.equal(got["colsum"], want["colsum"])
    if s > A.BLK:
        from deeplearningexamples_amd import functional as F
        st = torch.zeros(b * nh, s, 4, device=cuda)
        st[..., 0], st[..., 1] = want["mx"].reshape(b * nh, s).to(cuda), want["inv"].reshape(b * nh, s).to(cuda)
        wrong = (~want["mbytes"]).to(cuda)
        dq = F.attention_bwd(qkv.to(cuda), dctx.to(cuda), mask_add.to(cuda), st, b, s, nh, 0.125, p, SEED, OFF, keep_mask=wrong)
        assert torch.equal(G.bits(dq.cpu()), G.bits(want["dqkv"]))


def test_zz_report_ratios():
    for key in sorted(RATIOS):
        print("\n%s sigma %g: " % key + "  ".join("%s %.3f" % kv for kv in sorted(RATIOS[key].items())))
