"""The BERT row kernels of csrc/transformer.hip against fp64 references: LayerNorm forward / backward (with the fused
dropout + residual variants), masked softmax forward / backward (with and without dropout), the embedding gather-sum and
gradient scatter, the token-type select-sum and the row gather / scatter.  GPU only.

Every reference is plain torch on the CPU in float64, computed from the same 16-bit inputs the kernel read (seeded
torch.Generator, fp16 and bf16).  The shapes walk the kernels' dispatch: LayerNorm widths with 1, 2, 4 and 8 16-byte chunks per
lane and partial-chunk lanes (H not a multiple of 512), the FULL backward bodies (H = 512, 1024), 8 / 4 / 2 waves per backward
workgroup, forward rows past the first grid-stride lap, backward waves with 2-3 rows (the prefetched-row rotation and the clamped
read past the last row); softmax at every row length, with a partial last wave (`ok`) and a second grid-stride lap.

Bars.  u = 2^-24 (fp32 unit roundoff); ulp(v) = spacing of the 16-bit storage type at |v|.
* A 16-bit output rounded once lies within 0.5 ulp of the exact value.  fp32 arithmetic before that rounding adds an error e, so
  the stored value is within 1 ulp of the fp64 result rounded to 16 bits while |e| < 0.5 ulp, and within 1 ulp + |e| in general
  (outputs near 0, where the ulp is tiny).  e <= n u (sum of the magnitudes that entered), n the longest fp32 chain (Higham's
  gamma_n); 2 u |ref| more covers torch's fp64 -> 16-bit conversion, which rounds through fp32.
  - LayerNorm y: mean and variance are chains of 8 CH terms per lane + 6 shuffle levels (CH = 1 / 2 / 4 / 8 chunks per lane),
    so n = 8 CH + 16 covers them, rsqrt and the final multiply-add.  The magnitudes are |gamma xhat| + |beta| and
    |gamma| |mean| rstd: the fp32 mean carries an error of order u |mean|, which (z - mean) * rstd carries into xhat.
  - softmax P: the exponent s * scale + mask - max is formed in fp32 (error <= u (|v| + |max|) per step, times log2 e inside
    exp2) and the row sum is a chain of 8 + log2(L / 8) terms: e <= (3 (|v| + |max|) + 20) u P, plus 2^-126 because
    v_exp_f32 may flush a result below the smallest normal fp32 to zero.
* mean / rstd: the same chains give relative errors <= (8 CH + 8) u < 4.8e-6; bar 1e-5 (the mean's error relative to mean |z|:
  the mean of a row of random signs cancels).
* Column sums (dgamma, dbeta, dbias, select-sum, embedding gradient) are fp32 chains: error <= n u sum |terms| (plus the initial
  value with accumulate=True).  n is at most 3 rows per lane + 8 waves + 1 for the LayerNorm columns (bar 1e-5, 12 u would do);
  the select-sum uses its exact n = rows per group + groups + 2 (<= 166 here, < 1e-5 / u); the embedding scatter adds in an
  arbitrary order: (n_dup + 1) u, capped at 1e-5 where the worst case is larger (a random-order sum of n terms errs ~sqrt(n) u).
* dz (LayerNorm backward), dx and dS (softmax backward): one rounding to 16 bits is a relative error <= 2^-11 (fp16) / 2^-8
  (bf16) per element, so per row the relative L2 error is at most that, and the fp32 row reductions add ~n u.  Bars: 1e-3
  (fp16), 8e-3 (bf16); max error <= 2 ulp of the row's largest magnitude (0.5 ulp rounding + fp32 noise).
"""
import pytest
import torch

from deeplearningexamples_amd import functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
U = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
ROW_BAR = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
WIDTHS = [8, 256, 512, 768, 1000, 1024, 1032, 1536, 2048, 4096]
SOFTMAX_LENS = [8, 16, 32, 64, 128, 256, 512]
P_DROP = 0.1
EPS = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ulp(v, dtype):
    """Spacing of `dtype` at |v| (v float64, representable in dtype), subnormal spacing at and near 0."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype])


def _inv_keep(p):
    """1 / (1 - p) as make_drop (csrc/dropout.h) forms it: p quantised to 1/65536, fp32 division."""
    thr = min(max(int(p * 65536.0 + 0.5), 0), 65535)
    return torch.tensor(65536.0, dtype=torch.float32) / torch.tensor(float(65536 - thr), dtype=torch.float32)


def _pack_keep(keep):
    """bool keep mask -> the kernels' bit-packed bytes (bit k of byte i <-> flat element 8 i + k)."""
    b = keep.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)
    return b.sum(1).to(torch.uint8)


def _drop16(x16, keep, inv_keep):
    """dropout of a 16-bit tensor as the kernels do it: fp32 product with 1 / (1 - p), one rounding."""
    return torch.where(keep, x16.float() * inv_keep, torch.zeros((), dtype=torch.float32)).to(x16.dtype)


def _assert_ulp(got, ref, noise, what):
    """|got - ref rounded to got.dtype| <= 1 ulp of that value + noise + 2 u |ref|, elementwise (CPU tensors)."""
    assert torch.isfinite(got.double()).all(), what + ": non-finite output"
    r16 = ref.to(got.dtype).double()
    err = (got.double() - r16).abs()
    bar = _ulp(r16, got.dtype) + noise + 2 * U * ref.abs()
    bad = err > bar
    if bool(bad.any()):
        i = int(torch.argmax((err / bar).reshape(-1)))
        raise AssertionError("%s: %d of %d elements off; worst at flat index %d: got %r, fp64 %r, bar %r"
                             % (what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                float(bar.reshape(-1)[i])))


def _assert_rows(got, ref, dtype, what):
    """Per row: relative L2 error <= ROW_BAR[dtype], max error <= 2 ulp of the row's largest magnitude (CPU tensors)."""
    assert torch.isfinite(got.double()).all(), what + ": non-finite output"
    err = got.double() - ref
    en, rn = err.norm(dim=1), ref.norm(dim=1)
    bad = en > ROW_BAR[dtype] * rn
    if bool(bad.any()):
        r = int(torch.argmax(en / rn.clamp_min(1e-300)))
        raise AssertionError("%s: %d of %d rows above the relative L2 bar %g; worst row %d: %g"
                             % (what, int(bad.sum()), bad.numel(), ROW_BAR[dtype], r, float(en[r] / rn[r])))
    mx = err.abs().amax(1)
    lim = 2 * _ulp(ref.abs().amax(1).to(dtype).double(), dtype)
    bad = mx > lim
    if bool(bad.any()):
        r = int(torch.argmax(mx / lim))
        raise AssertionError("%s: %d rows with an element off by more than 2 ulp of the row's largest magnitude; row %d: %g > %g"
                             % (what, int(bad.sum()), r, float(mx[r]), float(lim[r])))


def _assert_colsum(got, ref, terms, rel, what):
    """|got - ref| <= rel * sum |terms|, elementwise (rel a number or a tensor)."""
    err = (got.double().cpu() - ref).abs()
    bar = rel * terms
    bad = err > bar
    if bool(bad.any()):
        i = int(torch.argmax((err / bar.clamp_min(1e-300)).reshape(-1)))
        raise AssertionError("%s: %d of %d sums off; worst at %d: got %r, fp64 %r, bar %r"
                             % (what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                float(bar.reshape(-1)[i])))


# ------------------------------------------------------------------ LayerNorm forward
def _chunks_per_lane(H):
    """CH template of ln_fwd_launch / ln_bwd_launch: 16-byte chunks per lane, rounded up to 1, 2, 4 or 8."""
    c = (H // 8 + 63) // 64
    return 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8


def _offset_row(g, H):
    return 256.0 + 4.0 * (torch.rand(H, generator=g) - 0.5)          # large common offset, spread 4


def _ln_inputs(g, rows, H):
    """x: normal rows; with 3 rows or more, rows 0 and rows-1 carry a large common offset and row 1 is constant."""
    x = torch.randn(rows, H, generator=g)
    res = 0.5 * torch.randn(rows, H, generator=g)
    if rows >= 3:
        x[0], x[rows - 1] = _offset_row(g, H), _offset_row(g, H)
        x[1], res[1] = 1.375, 0.0
    gamma = 1.0 + 0.5 * torch.randn(H, generator=g)
    beta = 0.5 * torch.randn(H, generator=g)
    return x, res, gamma, beta


def _run_ln_fwd(cuda, g, dtype, rows, H, variant):
    what = "layernorm_fwd %s %s H=%d rows=%d" % (variant, dtype, H, rows)
    x, res, gamma, beta = _ln_inputs(g, rows, H)
    x, res = x.to(dtype), res.to(dtype)
    xd, rd, gd, bd = x.to(cuda), res.to(cuda), gamma.to(cuda), beta.to(cuda)
    if variant == "plain":
        y, z, mean, rstd = F.layernorm_fwd(xd, gd, bd, eps=EPS)
        z16 = x
    elif variant == "residual":
        y, z, mean, rstd = F.layernorm_fwd(xd, gd, bd, residual=rd, eps=EPS)
        z16 = (x.float() + res.float()).to(dtype)
    else:
        y, z, mean, rstd, mask = F.dropout_add_layernorm_fwd(xd, gd, bd, rd, P_DROP, 11 + rows, 5 + H, eps=EPS)
        keep = F.unpack_dropout_mask(mask, x.shape).cpu()
        if keep.numel() >= 10000:
            assert abs(float(keep.float().mean()) - (1 - P_DROP)) < 0.02, what
        z16 = (_drop16(x, keep, _inv_keep(P_DROP)).float() + res.float()).to(dtype)
    y, z, mean, rstd = y.cpu(), z.cpu(), mean.cpu().double(), rstd.cpu().double()
    assert torch.equal(z, z16), what + ": z is not the 16-bit sum"
    zz = z16.double()
    mu = zz.mean(1, keepdim=True)
    rs = torch.rsqrt(((zz - mu) ** 2).mean(1, keepdim=True) + EPS)
    xh = (zz - mu) * rs
    g64, b64 = gamma.double(), beta.double()
    n = 8 * _chunks_per_lane(H) + 16
    noise = n * U * ((g64 * xh).abs() + b64.abs() + g64.abs() * mu.abs() * rs)
    if rows >= 3 and variant != "dropout":
        # constant row: zero variance, rstd = eps^-1/2, y = beta rounded, nothing non-finite
        assert torch.equal(y[1], beta.to(dtype)), what + ": constant row"
        noise[1] = 0.0
    _assert_ulp(y, xh * g64 + b64, noise, what + " y")
    _assert_colsum(mean, mu[:, 0], zz.abs().mean(1), 1e-5, what + " mean")
    _assert_colsum(rstd, rs[:, 0], rs[:, 0], 1e-5, what + " rstd")


@pytest.mark.parametrize("variant", ["plain", "residual", "dropout"])
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layernorm_fwd_vs_fp64(cuda, dtype, H, variant):
    """1 row, 3 rows (fewer than a workgroup's 4 waves), 301 rows; offset, constant and normal rows."""
    g = _gen(1000 + H)
    for rows in (1, 3, 301):
        _run_ln_fwd(cuda, g, dtype, rows, H, variant)


@pytest.mark.parametrize("variant", ["residual", "dropout"])
@pytest.mark.parametrize("H", [8, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layernorm_fwd_second_grid_lap(cuda, dtype, H, variant):
    """ln_fwd_launch caps the grid at 4096 workgroups x 4 waves: rows past 16384 take a second lap (the last row is an
    offset row)."""
    _run_ln_fwd(cuda, _gen(2000 + H), dtype, 4096 * 4 + 1001, H, variant)


# ------------------------------------------------------------------ LayerNorm backward
def _waves_per_group(H):
    return 8 if H <= 1024 else 4 if H <= 2048 else 2                 # ln_bwd_launch


def _bwd_rows(H):
    """Fewer rows than waves per workgroup; an odd count; more than 512 workgroups x waves, not a multiple of the waves
    (every wave gets 2 or 3 rows, the last prefetch clamps)."""
    nwv = _waves_per_group(H)
    return (max(nwv - 1, 1), 37, 8192 + 37 if nwv == 8 else 2501)


def _run_ln_bwd(cuda, g, dtype, rows, H, drop):
    what = "layernorm_bwd%s %s H=%d rows=%d" % (" +dropout" if drop else "", dtype, H, rows)
    z16 = (1.5 * torch.randn(rows, H, generator=g) + 0.3).to(dtype)
    if rows >= 3:
        z16[rows // 2] = _offset_row(g, H).to(dtype)
    dy16 = torch.randn(rows, H, generator=g).to(dtype)
    gamma = 1.0 + 0.5 * torch.randn(H, generator=g)
    zz, dy = z16.double(), dy16.double()
    # statistics from the test, in fp64, stored as fp32: the backward pass alone is under test
    mean32 = zz.mean(1).float()
    rstd32 = torch.rsqrt(((zz - zz.mean(1, keepdim=True)) ** 2).mean(1) + EPS).float()
    m, r = mean32.double()[:, None], rstd32.double()[:, None]
    xh = (zz - m) * r
    gg = dy * gamma.double()
    dz64 = r * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    dbeta64, dgamma64 = dy.sum(0), (dy * xh).sum(0)
    dbeta_t, dgamma_t = dy.abs().sum(0), (dy * xh).abs().sum(0)
    args = (dy16.to(cuda), z16.to(cuda), mean32.to(cuda), rstd32.to(cuda), gamma.to(cuda))
    inits = [torch.zeros(H), torch.zeros(H), torch.zeros(H)]
    for accumulate in (False, True):
        if accumulate:
            inits = [torch.randn(H, generator=g) for _ in range(3)]
        dg, db, dbias = (t.to(cuda, copy=True) for t in inits)
        if drop:
            keep = torch.rand(rows, H, generator=g) < 1 - P_DROP
            dz, dx = F.dropout_add_layernorm_bwd(*args, _pack_keep(keep).to(cuda), P_DROP, dg, db, dbias=dbias,
                                                 accumulate=accumulate)
        else:
            dz = F.layernorm_bwd(*args, dg, db, accumulate=accumulate)
        dz = dz.cpu()
        tag = what + (" accumulate" if accumulate else "")
        _assert_rows(dz, dz64, dtype, tag + " dz")
        d0, d1 = inits[0].double(), inits[1].double()
        _assert_colsum(dg, d0 + dgamma64, dgamma_t + d0.abs(), 1e-5, tag + " dgamma")
        _assert_colsum(db, d1 + dbeta64, dbeta_t + d1.abs(), 1e-5, tag + " dbeta")
        if drop:
            ik = _inv_keep(P_DROP)
            dx = dx.cpu()
            _assert_rows(dx, dz64 * keep.double() * float(ik), dtype, tag + " dx")
            assert torch.equal(dx, _drop16(dz, keep, ik)), tag + ": dx is not the rounded dz * keep / (1 - p)"
            d2 = inits[2].double()
            _assert_colsum(dbias, d2 + dx.double().sum(0), dx.double().abs().sum(0) + d2.abs(), 1e-5, tag + " dbias")


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layernorm_bwd_vs_fp64(cuda, dtype, H, drop):
    """dz (and dx) per row, dgamma / dbeta (/ dbias) column sums, accumulate off and on non-zero buffers."""
    g = _gen(3000 + H)
    for rows in _bwd_rows(H):
        _run_ln_bwd(cuda, g, dtype, rows, H, drop)


# ------------------------------------------------------------------ masked softmax
SCALE = float(torch.tensor(0.3, dtype=torch.float32))                # the fp32 scale the kernel multiplies by


def _softmax_mask(g, L, nb):
    """mask_add [nb, L] fp32: 0 on the first len_b columns, -10000 on the padded rest (one full, one length-1 batch)."""
    lens = torch.randint(1, L + 1, (nb,), generator=g)
    lens[0] = L
    if nb > 1:
        lens[1] = 1
    if nb > 2:
        lens[2] = L // 2 + 1
    return torch.where(torch.arange(L)[None, :] < lens[:, None], 0.0, -10000.0).float()


def _softmax_ref(s16, mask_add, rpb):
    rows = s16.shape[0]
    v = s16.double() * SCALE + mask_add.double()[torch.arange(rows) // rpb]
    mx = v.amax(1, keepdim=True)
    e = torch.exp(v - mx)
    return e / e.sum(1, keepdim=True), v, mx


def _softmax_shape(L):
    """3 sequences x 3 heads x (L - 1) query rows: rows is odd, never a multiple of the 64 / (L / 8) rows per wave (L < 512)."""
    heads, sq = 3, L - 1
    return 3 * heads * sq, heads * sq


def _run_softmax_fwd(cuda, g, dtype, L, rows, rpb, drop):
    what = "softmax_fwd%s %s L=%d rows=%d" % (" +dropout" if drop else "", dtype, L, rows)
    nb = (rows + rpb - 1) // rpb
    mask_add = _softmax_mask(g, L, nb)
    sigma = torch.full((rows, 1), 3.0)
    sigma[::2] = 400.0                     # scores * scale up to ~600: exp overflows fp32 without the max subtraction
    s16 = (torch.randn(rows, L, generator=g) * sigma).to(dtype)
    sd = s16.to(cuda, copy=True)
    if drop:
        dropped, mask = F.softmax_dropout_fwd_(sd, mask_add.to(cuda), rpb, SCALE, P_DROP, 17 + L, 3)
    else:
        F.softmax_fwd_(sd, mask_add.to(cuda), rpb, SCALE)
    p = sd.cpu()
    p64, v, mx = _softmax_ref(s16, mask_add, rpb)
    noise = (3 * (v.abs() + mx.abs()) + 20) * U * p64 + 2.0 ** -126
    _assert_ulp(p, p64, noise, what + " P")
    if drop:
        keep = F.unpack_dropout_mask(mask, p.shape).cpu()
        assert abs(float(keep.float().mean()) - (1 - P_DROP)) < 0.03, what
        assert torch.equal(dropped.cpu(), _drop16(p, keep, _inv_keep(P_DROP))), what + ": dropped != P * keep / (1 - p)"


def _run_softmax_bwd(cuda, g, dtype, L, rows, rpb, drop):
    what = "softmax_bwd%s %s L=%d rows=%d" % (" +dropout" if drop else "", dtype, L, rows)
    nb = (rows + rpb - 1) // rpb
    p16 = _softmax_ref((2.0 * torch.randn(rows, L, generator=g)).to(dtype), _softmax_mask(g, L, nb), rpb)[0].to(dtype)
    dp16 = torch.randn(rows, L, generator=g).to(dtype)
    dpd = dp16.to(cuda, copy=True)
    gr = dp16
    if drop:
        keep = torch.rand(rows, L, generator=g) < 1 - P_DROP
        F.softmax_dropout_bwd_(p16.to(cuda), dpd, _pack_keep(keep).to(cuda), SCALE, P_DROP)
        gr = _drop16(dp16, keep, _inv_keep(P_DROP))          # the kernel rounds the masked gradient to 16 bits first
    else:
        F.softmax_bwd_(p16.to(cuda), dpd, SCALE)
    p, gg = p16.double(), gr.double()
    ds64 = p * (gg - (gg * p).sum(1, keepdim=True)) * SCALE
    _assert_rows(dpd.cpu(), ds64, dtype, what + " dS")


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("L", SOFTMAX_LENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_fwd_vs_fp64(cuda, dtype, L, drop):
    rows, rpb = _softmax_shape(L)
    _run_softmax_fwd(cuda, _gen(4000 + L), dtype, L, rows, rpb, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("L", SOFTMAX_LENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_bwd_vs_fp64(cuda, dtype, L, drop):
    """dS = P (g - sum g P) scale, g = dP or its dropout backward rounded to 16 bits; P the 16-bit probabilities."""
    rows, rpb = _softmax_shape(L)
    _run_softmax_bwd(cuda, _gen(5000 + L), dtype, L, rows, rpb, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_second_grid_lap(cuda, dtype, drop):
    """L = 512 (1 row per wave): the grid is capped at 4096 workgroups x 4 waves, rows past 16384 take a second lap."""
    rows = 4096 * 4 + 617
    _run_softmax_fwd(cuda, _gen(6000), dtype, 512, rows, 1000, drop)
    _run_softmax_bwd(cuda, _gen(6001), dtype, 512, rows, 1000, drop)


# ------------------------------------------------------------------ embeddings, select-sum, row gather / scatter
@pytest.mark.parametrize("H,batch,seq", [(8, 3, 40), (768, 64, 128), (1032, 2, 128)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_embed_sum_bit_exact(cuda, dtype, H, batch, seq):
    """z = ((word[ids] + pos[t % S]) + type[tt]) in fp32, rounded once; ids include 0 and the last vocabulary row;
    64 x 128 tokens at H = 768 take the grid-stride loop past its first lap."""
    g = _gen(7000 + H)
    vocab, types = 1000, 3
    word, pos, typ = (torch.randn(n, H, generator=g) for n in (vocab, 512, types))
    ids = torch.randint(0, vocab, (batch * seq,), generator=g)
    ids[:3] = torch.tensor([vocab - 1, 0, vocab - 1])
    ids[-1] = vocab - 1
    tt = torch.randint(0, types, (batch * seq,), generator=g)
    z = F.embed_sum(word.to(cuda), pos.to(cuda), typ.to(cuda), ids.to(cuda), tt.to(cuda), seq, dtype)
    t = torch.arange(batch * seq)
    ref = ((word[ids] + pos[t % seq]) + typ[tt]).to(dtype)
    assert torch.equal(z.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_embed_scatter_add_vs_fp64(cuda, dtype):
    """gw[ids[t]] += dz[t] (fp32 atomics) onto a non-zero gradient, ids heavily duplicated ([PAD] = 0, [CLS] = 101)."""
    g = _gen(7100)
    vocab, H, tokens = 1000, 264, 4096
    ids = torch.randint(0, vocab, (tokens,), generator=g)
    u = torch.rand(tokens, generator=g)
    ids[u < 0.3] = 0
    ids[(u >= 0.3) & (u < 0.36)] = 101
    dz16 = torch.randn(tokens, H, generator=g).to(dtype)
    gw0 = torch.randn(vocab, H, generator=g)
    gw = gw0.to(cuda, copy=True)
    F.embed_scatter_add_(gw, dz16.to(cuda), ids.to(cuda))
    ref = gw0.double().index_add_(0, ids, dz16.double())
    terms = gw0.double().abs().index_add_(0, ids, dz16.double().abs())
    n = torch.bincount(ids, minlength=vocab).double()[:, None]
    _assert_colsum(gw, ref, terms, ((n + 1) * U).clamp_max(1e-5), "embed_scatter_add %s" % dtype)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rows_select_sum_vs_fp64(cuda, dtype, K):
    """out[k] (+)= sum of the rows with sel == k, around the 128-group split; H = 2056 spans two workgroup columns.  sel
    values outside [0, K) are dropped (documented at the kernel)."""
    g = _gen(7200 + K)
    for rows, H in ((1, 2056), (127, 2056), (128, 2056), (129, 2056), (128 * 37 + 5, 264)):
        x16 = torch.randn(rows, H, generator=g).to(dtype)
        sel = torch.randint(0, K, (rows,), generator=g)
        if rows > 100:
            sel[5], sel[77] = K, -1
        kept = (sel >= 0) & (sel < K)
        ref = torch.zeros(K, H, dtype=torch.float64).index_add_(0, sel[kept], x16.double()[kept])
        terms = torch.zeros(K, H, dtype=torch.float64).index_add_(0, sel[kept], x16.double().abs()[kept])
        rpb = (rows + 127) // 128
        n = rpb + (rows + rpb - 1) // rpb + 2                       # rows per group + groups + 2: the fp32 chain
        for accumulate in (False, True):
            out0 = torch.randn(K, H, generator=g) if accumulate else torch.zeros(K, H)
            out = F.rows_select_sum(x16.to(cuda), sel.to(cuda), K, out0.to(cuda, copy=True), accumulate=accumulate)
            r = ref + out0.double() if accumulate else ref
            _assert_colsum(out, r, terms + out0.double().abs(), n * U,
                           "rows_select_sum %s K=%d rows=%d accumulate=%s" % (dtype, K, rows, accumulate))


@pytest.mark.parametrize("H,n", [(8, 300), (1032, 5000)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rows_gather_scatter_bit_exact(cuda, dtype, H, n):
    """gather, scatter, scatter-accumulate ((dst + src) in fp32, rounded once: its own template instance per dtype); 5000
    rows at H = 1032 take the grid-stride loop past its first lap."""
    g = _gen(7300 + H)
    N = n + 777
    src = torch.randn(N, H, generator=g).to(dtype)
    idx = torch.randperm(N, generator=g)[:n]
    assert torch.equal(F.rows_gather(src.to(cuda), idx.to(cuda)).cpu(), src[idx])
    rows = torch.randn(n, H, generator=g).to(dtype)
    dst0 = torch.randn(N, H, generator=g).to(dtype)
    for accumulate in (False, True):
        dst = F.rows_scatter_(dst0.to(cuda, copy=True), rows.to(cuda), idx.to(cuda), accumulate=accumulate).cpu()
        ref = dst0.clone()
        ref[idx] = (dst0[idx].float() + rows.float()).to(dtype) if accumulate else rows
        assert torch.equal(dst, ref), "rows_scatter_ accumulate=%s" % accumulate


# ------------------------------------------------------------------ argument errors
def test_argument_errors(cuda):
    """Shapes outside the kernels' envelopes are refused before any launch."""
    dt = torch.float16
    bad = (ValueError, RuntimeError)

    def ln(h, rows=4):
        x = torch.zeros(rows, h, dtype=dt, device=cuda)
        return x, torch.ones(h, device=cuda), torch.zeros(h, device=cuda)

    for h in (12, 4104):                                            # H not a multiple of 8; H > 4096
        x, gm, bt = ln(h)
        st = torch.zeros(4, device=cuda)
        with pytest.raises(bad):
            F.layernorm_fwd(x, gm, bt)
        with pytest.raises(bad):
            F.dropout_add_layernorm_fwd(x, gm, bt, x, 0.1, 1, 2)
        with pytest.raises(bad):
            F.layernorm_bwd(x, x, st, st, gm, torch.zeros_like(gm), torch.zeros_like(gm))
        with pytest.raises(bad):
            F.dropout_add_layernorm_bwd(x, x, st, st, gm, torch.zeros(4 * h // 8, dtype=torch.uint8, device=cuda), 0.1,
                                        torch.zeros_like(gm), torch.zeros_like(gm))
    for L in (4, 96, 1024):                                         # outside 8 ... 512, or not a power of two
        s = torch.zeros(8, L, dtype=dt, device=cuda)
        madd = torch.zeros(1, L, device=cuda)
        with pytest.raises(bad):
            F.softmax_fwd_(s, madd, 8, 1.0)
        with pytest.raises(bad):
            F.softmax_dropout_fwd_(s, madd, 8, 1.0, 0.1, 1, 2)
        with pytest.raises(bad):
            F.softmax_bwd_(s, s.clone(), 1.0)
        with pytest.raises(bad):
            F.softmax_dropout_bwd_(s, s.clone(), torch.zeros(8 * L // 8, dtype=torch.uint8, device=cuda), 1.0, 0.1)
    x = torch.zeros(16, 64, dtype=dt, device=cuda)
    sel = torch.zeros(16, dtype=torch.int64, device=cuda)
    for k in (0, 5):                                                # K outside 1 ... 4
        with pytest.raises(bad):
            F.rows_select_sum(x, sel, k, torch.zeros(max(k, 1), 64, device=cuda))
    x, gm, bt = ln(64)
    s = torch.zeros(8, 64, dtype=dt, device=cuda)
    madd = torch.zeros(1, 64, device=cuda)
    st = torch.zeros(4, device=cuda)
    mask = torch.zeros(4 * 64 // 8, dtype=torch.uint8, device=cuda)
    with pytest.raises(bad):                                        # p = 1
        F.dropout_add_layernorm_fwd(x, gm, bt, x, 1.0, 1, 2)
    with pytest.raises(bad):
        F.softmax_dropout_fwd_(s, madd, 8, 1.0, 1.0, 1, 2)
    with pytest.raises(bad):
        F.dropout_add_layernorm_bwd(x, x, st, st, gm, mask, 1.0, torch.zeros_like(gm), torch.zeros_like(gm))
    # rows = 0: the forward is a no-op, the backward refuses it (it has column sums to finish)
    x0, gm, bt = ln(64, rows=0)
    y, _, _, _ = F.layernorm_fwd(x0, gm, bt)
    assert y.shape == (0, 64)
    with pytest.raises(bad):
        F.layernorm_bwd(x0, x0, st[:0], st[:0], gm, torch.zeros_like(gm), torch.zeros_like(gm))
