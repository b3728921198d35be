"""The kernels of csrc/transformer_xl.hip through deeplearningexamples_amd.functional and the C ABI.  GPU only.

dle_txl_rel_attention_fwd.  Shapes (B, heads, qlen, mlen): (1,1,1,0) (2,3,5,0) (1,2,8,20) (3,2,64,0) (2,2,64,64) (2,1,37,91)
(1,2,64,640) (1,1,128,200) (1,1,128,1600), fp16 and bf16; shift in {none, 1, max(1, qlen - 3)}; the ring tight (cap = klen, start
in the middle so the window wraps) or slack (cap = klen + 37, start chosen so that the wrap falls inside a key tile).  ctx is a
view at the head of a NaN-filled buffer (tests/_exact_grid.Out): the tail keeps its bits, every element is written.

EXACT CASES (bit for bit, +0 = -0).
* Selector by distance.  K = 0; q = e_0 - v on a k/4 grid, so b = round16(q + v) = e_0 exactly; r[d] = G [d == d*] e_0 with G = 1024
  and scale = 1/8: score(i, j) = 128 where i + mlen - j == d* and 0 elsewhere.  128 >= GAP = 104 of tests/_attention_reference.py:
  an fp32 exp of -128 is exactly 0, also as the online rescale factor and as a partial result's merge factor, so every query
  whose key i + mlen - d* is allowed returns that key's V row exactly (V on a k/4 grid: the merge adds exact zeros).  Run for d*
  over EVERY distance 0 .. klen - 1 of the shape.  This pins the skew (which r row meets which key), the ring arithmetic of V and
  both band edges (a query whose selected key is masked is not checked, but must be finite).
* Selector by key (the mirror).  r = 0; q = e_0 - u, so a = e_0; K_j = G [j == j*] e_0: every query that may see j* returns V_j*.
  j* over EVERY key: the ring arithmetic of K.
  For klen <= 128 every (shift, ring) pair runs every d* / j*; above that the six pairs rotate over d* / j* (every distance and
  key runs, every pair runs on a sixth of them) to keep a case within seconds.  The comparison happens on the device; one read per case.
* Out-of-window rows: NaN in every physical ring row outside the logical window (slack ring) leaves the output bits unchanged.

RANDOM INPUTS against float64 (tests/_txl_ref.attn_reference) under a DERIVED per-element bar (attn_bar), sigma 1 and 3.
u = 2^-24, m = 10 / 7 mantissa bits.  The reference forms a = round16(fp32(q) + fp32(u)) and b likewise, as the kernel's contract
states them: these two roundings are part of the function, an IEEE fp32 sum followed by one conversion, so they are in the
reference and need no term of the bar.  For ctx[i, d] = sum_j P_ij V_jd the kernel rounds two kinds of things to 16 bits, the
probability operand of the second contraction and the stored output, and keeps everything else in fp32:
    |got - ref| <= sum_j rnd(P_ij) |V_jd|       one rounding of the operand, rnd(P) = max(2^-(m+1) P, half the subnormal spacing): the
                                                kernel rounds exp(s - m_partial) with m_partial <= the row maximum and rescales by
                                                factors <= 1 / l with l >= 1, so the absolute term is not exceeded
                 + n u M                        fp32 accumulation, M = sum_j P |V|, n = 3 ceil(klen / 32) + 16: two matrix-instruction
                                                accumulations and one rescale product per key tile, the merge of four partials
                 + sum_j E_ij P_ij |V_jd|       the fp32 probability: E = e_p + e_l on allowed keys with
                     e_s = 11 u scale (sum_d |a||K| + sum_d |b||r|)     a score is 128 products in eight matrix-instruction
                                                                        accumulations, one sum of the two terms, one product
                     e_p = (3 (|s| + |max|) + 20) u                     the exponential (tests/test_gpu_bert_rowops)
                           + w (6 A + 20) u                             w = ceil(tiles / 4) + 1 rescale / merge factors exp(dm),
                                                                        |dm| <= 2 A, A the row's largest allowed |score|
                           + e_s
                     e_l = sum_j P e_p + (18 w + 8) u                   the row sum: its terms' errors and its fp32 chain
                 + 1 ulp16(ref) + 2 u |ref|     the stored rounding (the fp32 value may sit across a tie), torch's conversion
tests/test_txl_host.py checks this bar on the CPU: an fp32 model of the kernel's arithmetic stays below 0.6 x, planted faults (skew
off by one, either band edge, a stale maximum, the ring start) leave it by factors of 10 to 10^4.
Worst |error| / bar on the MI355X over the nine shapes, both types, sigma 1 and 3 (a record; the pass condition is <= 1): 0.62;
every exact case passed bit for bit on the first run.

Small kernels.  dle_txl_kv_append bit for bit across the wrap, the rest of the ring untouched.  dle_rows_gather_scale bit for bit
against float64 rounded once (fp32 x * scale is one rounding of the exact product of a 16-bit value and an fp32 scale held as such;
the double rounding fp32 -> 16 bits is avoided by power-of-two and k/8 scales), duplicated source rows, both optional lists,
widths 16 and 1024.  dle_row_nll against float64: bar = (n_classes / 256 + 16 + 8) u sum-relative on the sum of exponentials (a
chain of n / 256 terms per thread, the wavefront and block reductions), i.e. |lse error| <= that + (3 |max| + 20) u per term,
plus u (|max| + |log sum| + |logit_target|) for the three-term result and the accumulate sum: bar = (n / 256 + 60) u
(1 + |max| + |lse| + |x_t| + |previous|); classes 2, 103 and 160003, accumulate, a permuted pos, a row whose maximum is its last class.

Argument checks: every entry point raises without a launch (the attention launch counter and the destination bits unchanged).
"""
import functools
import math

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests import _exact_grid as G
from tests import _txl_ref as R
from tests._attention_reference import GAP

pytestmark = pytest.mark.gpu

HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
SHAPES = [(1, 1, 1, 0), (2, 3, 5, 0), (1, 2, 8, 20), (3, 2, 64, 0), (2, 2, 64, 64), (2, 1, 37, 91), (1, 2, 64, 640), (1, 1, 128, 200),
          (1, 1, 128, 1600)]
SHAPE_IDS = ["B%dh%dq%dm%d" % s for s in SHAPES]
SCALE, BIG = 0.125, 1024.0
assert BIG * SCALE >= GAP
DEV = "cuda"


def run_attention(qkv, u, v, kv, r, nh, qlen, mlen, start, shift, scale=SCALE):
    """Through functional into a guarded output -> ctx [B*qlen, H] on the device."""
    b, h = kv.shape[0], nh * 64
    out = G.Out((b * qlen, h), qkv.dtype, DEV)
    before = F.txl_attention_launch_count()
    F.txl_rel_attention_fwd(qkv[:, :h], u, v, kv, r, nh, qlen, mlen, start, shift, scale, out=out.t)
    assert F.txl_attention_launch_count() == before + 1
    return out


def heads(ctx, b, qlen, nh):
    return ctx.view(b, qlen, nh, 64).permute(0, 2, 1, 3)


def grid(shape, seed, dtype, kmax=8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-kmax, kmax + 1, shape, generator=g).float() / 4).to(dtype)


def combos(qlen, mlen):
    return [(s, c) for s in R.shift_choices(qlen) for c in R.ring_configs(qlen, mlen)]


@pytest.mark.parametrize("mirror", [False, True], ids=["by_distance", "by_key"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_selector_exact(shape, dtype, mirror):
    b, nh, qlen, mlen = shape
    klen, h = qlen + mlen, nh * 64
    V = grid((b, klen, h), 3, dtype)
    bias = grid((nh, 64), 4, dtype, 4)                       # v (by distance) or u (by key): q + bias = e_0 exactly
    other = grid((nh, 64), 5, dtype, 4)
    e0 = torch.zeros(nh, 64)
    e0[:, 0] = 1.0
    qkv = torch.zeros(b * qlen, 3 * h, dtype=dtype)
    qkv[:, :h] = (e0 - bias.float()).to(dtype).reshape(1, h)
    assert torch.equal((qkv[:, :h].float() + bias.float().reshape(1, h)), e0.reshape(1, h).expand(b * qlen, h))
    u, v = (other, bias) if not mirror else (bias, other)
    qkv_d, u_d, v_d, V_d = qkv.to(DEV), u.to(DEV), v.to(DEV), V.to(DEV)
    Vh = V_d.view(b, klen, nh, 64).permute(0, 2, 1, 3)                                     # [b, nh, klen, 64]
    ii = torch.arange(qlen, device=DEV)
    cs = combos(qlen, mlen)
    rings = {}
    for shift, (cap, start) in cs:
        if (cap, start) not in rings:
            rings[(cap, start)] = R.ring_of(torch.zeros(b, klen, h, dtype=dtype), V, cap, start, 0.0).to(DEV)
    r_d = torch.zeros(klen, h, dtype=dtype, device=DEV)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    checked = torch.zeros((), dtype=torch.int64, device=DEV)
    phys_all = torch.arange(klen, device=DEV)
    for sel in range(klen):
        todo = cs if klen <= 128 else [cs[sel % len(cs)]]
        for shift, (cap, start) in todo:
            kv = rings[(cap, start)]
            if not mirror:
                r_d[sel, 0::64] = BIG
                jstar = ii + mlen - sel                                                    # per query
            else:
                kv[:, (start + sel) % cap, 0:h:64] = BIG
                jstar = torch.full_like(ii, sel)
            out = run_attention(qkv_d, u_d, v_d, kv, r_d, nh, qlen, mlen, start, shift)
            got = heads(out.check("txl_rel_attention_fwd ctx"), b, qlen, nh)
            ok = (jstar >= 0) & (jstar <= ii + mlen) & (ii - shift < jstar)
            want = Vh[:, :, jstar.clamp(0, klen - 1)]                                      # [b, nh, qlen, 64]
            bad += ((got != want) & ok[None, None, :, None]).sum()
            bad += (~torch.isfinite(got.float())).sum()
            checked += ok.sum()
            if not mirror:
                r_d[sel, 0::64] = 0
            else:
                kv[:, (start + sel) % cap, 0:h:64] = 0
    bad, checked = int(bad), int(checked)
    print("selector %s %s: %d rows checked" % (shape, "by key" if mirror else "by distance", checked))
    assert checked > 0 and bad == 0, "%d elements differ from the selected V row (or are not finite)" % bad


@functools.lru_cache(maxsize=None)
def generic_case(shape, dtype, sigma):
    b, nh, qlen, mlen = shape
    inp = R.attn_inputs(b, nh, qlen, mlen, dtype, 11 + qlen + mlen, sigma)
    refs = {}
    for shift in R.shift_choices(qlen):
        ref = R.attn_reference(inp, shift, SCALE)
        refs[shift] = (ref["ctx"], R.attn_bar(ref, dtype))
    return inp, refs


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_random_inputs_against_float64(shape, dtype, sigma):
    b, nh, qlen, mlen = shape
    inp, refs = generic_case(shape, dtype, sigma)
    worst = 0.0
    for shift, (cap, start) in combos(qlen, mlen):
        kv = R.ring_of(inp["K"], inp["V"], cap, start, 0.0).to(DEV)
        out = run_attention(inp["qkv"].to(DEV), inp["u"].to(DEV), inp["v"].to(DEV), kv, inp["r"].to(DEV), nh, qlen, mlen, start, shift)
        got = heads(out.check("txl_rel_attention_fwd ctx"), b, qlen, nh).cpu().double()
        assert bool(torch.isfinite(got).all()), "an element was not written"
        ref, bar = refs[shift]
        ratio = float(((got - ref).abs() / bar).max())
        print("%s %s sigma %g shift %d ring (%d, %d): worst |error| / bar %.3f" % (shape, dtype, sigma, min(shift, 9999), cap, start, ratio))
        worst = max(worst, ratio)
    assert worst <= 1.0, "worst |error| / bar %.3f" % worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_out_of_window_rows_do_not_matter(shape, dtype):
    b, nh, qlen, mlen = shape
    inp, _ = generic_case(shape, dtype, 1.0)
    for shift in R.shift_choices(qlen):
        cap, start = R.ring_configs(qlen, mlen)[1]
        outs = []
        for fill in (0.0, float("nan")):
            kv = R.ring_of(inp["K"], inp["V"], cap, start, fill).to(DEV)
            assert fill == 0.0 or int(torch.isnan(kv.float()).all(-1).sum()) == b * (cap - qlen - mlen)
            out = run_attention(inp["qkv"].to(DEV), inp["u"].to(DEV), inp["v"].to(DEV), kv, inp["r"].to(DEV), nh, qlen, mlen, start, shift)
            outs.append(G.bits(out.check("ctx")).cpu())
        assert torch.equal(outs[0], outs[1]), "NaN outside the logical window changed the output (shift %d)" % shift


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,h,qlen,mlen,cap,start", [(2, 128, 8, 20, 28, 5), (3, 64, 3, 20, 28, 27), (1, 192, 64, 0, 64, 0), (2, 64, 5, 7, 49, 40)])
def test_kv_append_exact(dtype, b, h, qlen, mlen, cap, start):
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(b * qlen, 3 * h, generator=g).to(dtype).to(DEV)
    kv0 = torch.randn(b, cap, 2 * h, generator=g).to(dtype)
    out = G.Out((b, cap, 2 * h), dtype, DEV, fill=kv0.to(DEV))
    F.txl_kv_append(qkv, out.t, qlen, mlen, start)
    got = out.check("txl_kv_append").cpu()
    want = kv0.clone()
    rows = (start + mlen + torch.arange(qlen)) % cap
    want[:, rows] = qkv.cpu().view(b, qlen, 3 * h)[:, :, h:]
    G.assert_same(G.bits(got), G.bits(want), "txl_kv_append")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [16, 1024])
@pytest.mark.parametrize("lists", ["both", "src", "dst", "none"])
def test_rows_gather_scale_exact(dtype, width, lists):
    g = torch.Generator().manual_seed(9)
    n_src, n_dst, rows = 37, 41, 29
    src = torch.randn(n_src, width, generator=g).to(dtype)
    dst0 = torch.randn(n_dst, width, generator=g).to(dtype)
    src_idx = torch.randint(0, n_src, (rows,), generator=g).to(torch.int32) if lists in ("both", "src") else None
    if src_idx is not None:
        src_idx[5] = src_idx[6] = src_idx[0]                                          # duplicated source rows
    dst_idx = torch.randperm(n_dst, generator=g)[:rows].to(torch.int32) if lists in ("both", "dst") else None
    for scale in (1.0, 11.375, math.sqrt(512.0)):
        out = G.Out((n_dst, width), dtype, DEV, fill=dst0.to(DEV))
        F.rows_gather_scale(src.to(DEV), out.t, rows, src_idx=None if src_idx is None else src_idx.to(DEV),
                            dst_idx=None if dst_idx is None else dst_idx.to(DEV), scale=scale)
        got = out.check("rows_gather_scale").cpu()
        si = src_idx.long() if src_idx is not None else torch.arange(rows)
        di = dst_idx.long() if dst_idx is not None else torch.arange(rows)
        want = dst0.clone()
        # the kernel's contract: one fp32 product of the value and the fp32 scale, one conversion
        want[di] = (src[si].float() * torch.tensor(scale, dtype=torch.float32)).to(dtype)
        if scale in (1.0, 11.375):
            # a k/8 scale times a 16-bit value is exact in fp32: equal to float64 rounded once
            assert torch.equal(want[di], (src[si].double() * scale).to(dtype))
        G.assert_same(G.bits(got), G.bits(want), "rows_gather_scale width %d lists %s scale %g" % (width, lists, scale))


@pytest.mark.parametrize("n_classes", [2, 103, 160003])
def test_row_nll_against_float64(n_classes):
    g = torch.Generator().manual_seed(n_classes)
    rows, ld = 7, n_classes + (5 if n_classes < 1000 else 0)
    logits = 4.0 * torch.randn(rows, ld, generator=g)
    logits[2, n_classes - 1] = 40.0                                                    # the maximum sits in the last class
    logits[:, n_classes:] = float("nan")                                             # columns past n_classes are not read
    target = torch.randint(0, n_classes, (rows,), generator=g).to(torch.int32)
    target[2], target[3] = n_classes - 1, 0
    pos = torch.randperm(rows + 3, generator=g)[:rows].to(torch.int32)
    prev = torch.randn(rows + 3, generator=g)
    x = logits[:, :n_classes].double()
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, target.long()[:, None]).squeeze(1)
    ref = lse - xt
    bar0 = (n_classes / 256 + 60) * R.U32 * (1 + x.amax(1).abs() + lse.abs() + xt.abs())
    for accumulate in (False, True):
        for use_pos in (False, True):
            out = G.Out((rows + 3,), torch.float32, DEV, fill=prev.to(DEV))
            F.row_nll(logits.to(DEV), target.to(DEV), out.t, pos=pos.to(DEV) if use_pos else None, n_classes=n_classes, accumulate=accumulate)
            got = out.check("row_nll").cpu()
            where = pos.long() if use_pos else torch.arange(rows)
            want = ref + (prev[where].double() if accumulate else 0.0)
            bar = bar0 + (R.U32 * (prev[where].abs().double() + want.abs()) if accumulate else 0.0)
            ratio = float(((got[where].double() - want).abs() / bar).max())
            print("row_nll %d classes accumulate %s pos %s: worst |error| / bar %.3f" % (n_classes, accumulate, use_pos, ratio))
            assert ratio <= 1.0
            rest = torch.ones(rows + 3, dtype=torch.bool)
            rest[where] = False
            assert torch.equal(G.bits(got[rest]), G.bits(prev[rest])), "row_nll wrote a position it was not given"


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_without_a_launch():
    dt = HF
    b, nh, qlen, mlen, cap = 2, 2, 8, 20, 28
    h = nh * 64
    z = lambda *s, d=dt: torch.zeros(*s, dtype=d, device=DEV)
    qkv, u, v, kv, r = z(b * qlen, 3 * h), z(nh, 64), z(nh, 64), z(b, cap, 2 * h), z(cap, h)
    out = G.Out((b * qlen, h), dt, DEV)
    before = F.txl_attention_launch_count()
    good = dict(q=qkv[:, :h], u=u, v=v, kv=kv, r=r, heads=nh, qlen=qlen, mlen=mlen, start=3, shift=qlen, scale=SCALE, out=out.t)
    bad = [dict(qlen=513), dict(mlen=21), dict(start=cap), dict(start=-1), dict(shift=0), dict(r=z(cap - 1, h)), dict(u=z(nh, 32)),
           dict(kv=z(b, cap, 2 * h, d=BF)), dict(q=z(b * qlen, 3 * h)[:, 1:h + 1]), dict(q=z(b * qlen + 1, h)), dict(heads=3),
           dict(kv=z(b, 4097, 2 * h), mlen=4090), dict(q=qkv[:, :h].cpu())]
    for change in bad:
        with pytest.raises((ValueError, C.DleError)):
            F.txl_rel_attention_fwd(**dict(good, **change))
    # the C ABI's own checks: -1 and a message, nothing launched
    lib = C.lib()
    args = [C.ptr(qkv), 3 * h, C.ptr(u), C.ptr(v), C.ptr(kv), C.ptr(r), C.ptr(out.t), b, nh, 64, qlen, mlen, cap, 3, cap, qlen, SCALE, C.F16, C.stream()]
    for pos, val in ((9, 32), (10, 0), (10, 513), (11, -1), (12, qlen + mlen - 1), (12, 4097), (13, cap), (14, qlen + mlen - 1), (15, 0),
                     (17, C.F32), (1, 3 * h + 4), (0, C.ptr(qkv) + 2), (6, 0)):
        a = list(args)
        a[pos] = val
        assert lib.dle_txl_rel_attention_fwd(*a) == -1 and lib.dle_last_error()
    assert lib.dle_txl_attention_supported(512, 4096, 64) == 1
    assert [lib.dle_txl_attention_supported(*a) for a in ((0, 8, 64), (513, 600, 64), (8, 4097, 64), (8, 7, 64), (8, 8, 32))] == [0] * 5
    torch.cuda.synchronize()
    assert F.txl_attention_launch_count() == before
    assert bool(torch.isnan(out.check("ctx").float()).all()), "a rejected call wrote its output"

    ring = G.Out((b, cap, 2 * h), dt, DEV)
    for change in (dict(qlen=9), dict(mlen=21), dict(start=cap), dict(qkv=z(b * qlen, 3 * h + 8)), dict(kv=z(b, cap, 2 * h, d=BF))):
        kw = dict(dict(qkv=qkv, kv=ring.t, qlen=qlen, mlen=mlen, start=0), **change)
        with pytest.raises((ValueError, C.DleError)):
            F.txl_kv_append(**kw)
    assert lib.dle_txl_kv_append(C.ptr(qkv), 3 * h, C.ptr(ring.t), b, h, qlen, mlen, cap, cap, C.F16, C.stream()) == -1
    assert lib.dle_txl_kv_append(C.ptr(qkv), 3 * h - 8, C.ptr(ring.t), b, h, qlen, mlen, cap, 0, C.F16, C.stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(ring.check("kv").float()).all())

    src, dst = z(10, 16), G.Out((10, 16), dt, DEV)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=DEV)
    for kw in (dict(rows=11), dict(rows=2, src_idx=i32(0, 1, 2)), dict(rows=2, src_idx=torch.zeros(2, dtype=torch.int64, device=DEV)),
               dict(rows=2, src=z(10, 12)), dict(rows=2, src=z(10, 16, d=BF)), dict(rows=-1)):
        kw = dict(dict(src=src, dst=dst.t), **kw)
        with pytest.raises((ValueError, C.DleError)):
            F.rows_gather_scale(**kw)
    assert lib.dle_rows_gather_scale(C.ptr(src), 0, C.ptr(dst.t), 0, 11, 16, 16, 16, 10, 10, 1.0, C.F16, C.stream()) == -1
    assert lib.dle_rows_gather_scale(C.ptr(src), 0, C.ptr(dst.t), 0, 2, 12, 16, 16, 10, 10, 1.0, C.F16, C.stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst.check("dst").float()).all())

    logits, nll = torch.zeros(4, 10, device=DEV), G.Out((4,), torch.float32, DEV)
    tgt = i32(0, 1, 2, 3)
    for kw in (dict(n_classes=11), dict(n_classes=0), dict(target=i32(0, 1, 2)), dict(pos=i32(0, 1, 2)), dict(logits=logits.half()),
               dict(nll=torch.zeros(3, device=DEV))):
        kw = dict(dict(logits=logits, target=tgt, nll=nll.t), **kw)
        with pytest.raises((ValueError, C.DleError)):
            F.row_nll(**kw)
    assert lib.dle_row_nll(C.ptr(logits), 10, C.ptr(tgt), 0, C.ptr(nll.t), 4, 160004, 4, 0, C.stream()) == -1
    assert lib.dle_row_nll(C.ptr(logits), 10, C.ptr(tgt), 0, C.ptr(nll.t), 5, 10, 4, 0, C.stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(nll.check("nll")).all())
    # rows whose index, target or position is out of range are skipped, not written
    F.row_nll(logits, i32(0, 10, -1, 3), nll.t, pos=i32(0, 1, 2, 4))
    F.rows_gather_scale(src, dst.t, 3, src_idx=i32(0, 10, -1), dst_idx=i32(10, 1, 2))
    torch.cuda.synchronize()
    assert torch.isnan(nll.check("nll")).tolist() == [False, True, True, True]
    assert bool(torch.isnan(dst.check("dst").float()).all())
