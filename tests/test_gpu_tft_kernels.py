"""The kernels of csrc/tft.hip through deeplearningexamples_amd.functional and the C ABI, fp16 and bf16.  GPU only.

Random inputs are compared with the float64 statement of tests/_tft_ref.py under its propagated per-element bar (mode 'bar': the
docstring there states every rule); each such test prints its worst |error| / bar.  The kernels have no grid-stride loop: a
workgroup owns 32 rows (GRN, VSN), 32 batch rows (LSTM) or 32 queries of one batch element (attention), so the row counts are 1,
31, 32, 33 and 100 (four workgroups, the last one partial).

Exact cases (bit for bit):
* GRN, GLU weights zero and a bias of -40 / +40 on the gate half: sigmoid is 4e-18 or exactly 1 in fp32, so the sum in front of the
  LayerNorm is the residual alone, or the residual plus the bias of the value half.  With rows of +-c the mean is exactly 0 and the
  variance exactly c^2: the output is +-c / sqrt(c^2 + 1e-3) (gamma 1, beta 0) rounded once.
* GRN gate mode with an identity value half on k/4 grid inputs (tests/_exact_grid): a = x exactly, x + res = +-2.
* VSN with one variable: the weight is exactly 1.0.  (The one-categorical static case of the model IS dle_tft_grn_fwd with a row
  index list; test_grn_gather checks that path bit for bit against the same rows gathered by torch.)
* LSTM with W_hh = 0: per step the cell is elementwise in the chosen pre-activations; 0 / +-40 pre-activations make every gate
  exactly 0, 1/2 or 1 and tanh(+-40) = +-1, so c and h follow an exact recurrence.
* LSTM state hand-off (T = 9 against 6 then 3) and a batch row alone against the row in its batch.
* Attention selector: one key carries a large score in every head, so the output is that key's V row through out_proj, for every
  key position; a key just behind the mask is never selected.  Equal scores: the exact uniform mean 1 / (position + 1).

Worst |error| / bar on the MI355X (a record; the pass condition is <= 1; each test prints its own): GRN 0.31 (gate mode 0.21),
VSN 0.30 (selection weights 0.12), LSTM 0.38 over the steps, attention 0.32 (probabilities 0.03).  Every exact case held bit for bit
on the first run.
"""
import math

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests import _exact_grid as G
from tests import _tft_ref as R

pytestmark = pytest.mark.gpu

HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
ROWS = [1, 31, 32, 33, 100]
DEV = "cuda"
H = 128


def dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def under_bar(got, ref, what):
    err = (got.double().cpu() - ref.v).abs()
    ratio = float((err / ref.bar()).max())
    print("%s: worst |error| / bar = %.3f (largest |error| %.3g)" % (what, ratio, float(err.max())))
    assert torch.isfinite(got.float()).all(), what
    assert ratio <= 1.0, "%s: %.3f of the bar" % (what, ratio)


def f64(p):
    return {k: v.double() for k, v in p.items()}


# ---- GRN ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", ROWS)
def test_grn_random(rows, dtype):
    M = R.Mode("bar", dtype)
    x = R.randn16((rows, H), 1, dtype)
    # plain and with a context row for every 3 rows
    for ctx_on in (False, True):
        p = R.grn_params(2 + ctx_on, dtype, ctx=ctx_on)
        ctx = R.randn16(((rows + 2) // 3, H), 4, dtype) if ctx_on else None
        out = G.Out((rows, H), dtype, DEV)
        F.tft_grn_fwd(x.to(DEV), dev(p), ctx=ctx.to(DEV) if ctx_on else None, rows_per_ctx=3, out=out.t)
        ref, _ = R.grn(M, R.V(x), f64(p), ctx=R.V(ctx) if ctx_on else None, rows_per_ctx=3)
        under_bar(out.check("tft_grn_fwd"), ref, "grn rows %d ctx %d" % (rows, ctx_on))
    # gate mode, dense residual, with the quantile tail
    p = R.grn_params(5, dtype, gate=True)
    res = R.randn16((rows, H), 6, dtype)
    g = torch.Generator().manual_seed(7)
    wq, bq = torch.randn(3, H, generator=g) / math.sqrt(H), 0.1 * torch.randn(3, generator=g)
    out, q = F.tft_grn_fwd(x.to(DEV), dev(p), res=res.to(DEV), wq=wq.to(DEV), bq=bq.to(DEV))
    ref, rq = R.grn(M, R.V(x), f64(p), res=R.V(res), wq=wq, bq=bq)
    under_bar(out, ref, "gate rows %d" % rows)
    under_bar(q, rq, "gate tail rows %d" % rows)
    q_only = F.tft_grn_fwd(x.to(DEV), dev(p), res=res.to(DEV), wq=wq.to(DEV), bq=bq.to(DEV), want_out=False)
    assert torch.equal(q_only, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grn_gate_strided_residual(dtype):
    """The residual as the last `steps` steps of every batch element of a [B, T, 128] tensor (attention_gate / decoder_gate)."""
    B, T, steps = 7, 9, 5
    x = R.randn16((B * steps, H), 11, dtype).to(DEV)
    full = R.randn16((B, T, H), 12, dtype).to(DEV)
    p = dev(R.grn_params(13, dtype, gate=True))
    a = F.tft_grn_fwd(x, p, res=full, res_rows_per_batch=steps)
    b = F.tft_grn_fwd(x, p, res=full[:, T - steps:].reshape(B * steps, H).contiguous())
    G.assert_same(G.bits(a), G.bits(b), "strided residual")


@pytest.mark.parametrize("dtype", DTYPES)
def test_grn_gather(dtype):
    table = R.randn16((11, H), 21, dtype).to(DEV)
    idx = torch.tensor([3, 0, 10, 3, 7] * 8, dtype=torch.int32, device=DEV)
    p = dev(R.grn_params(22, dtype))
    a = F.tft_grn_fwd(table, p, x_index=idx)
    b = F.tft_grn_fwd(table[idx.long()].contiguous(), p)
    G.assert_same(G.bits(a), G.bits(b), "gathered rows")
    bad = idx.clone()
    bad[1], bad[2] = 11, -1                                         # outside the table: a zero row, nothing read
    c = F.tft_grn_fwd(table, p, x_index=bad)
    z = F.tft_grn_fwd(torch.zeros(1, H, dtype=dtype, device=DEV), p)
    G.assert_same(G.bits(c[1]), G.bits(z[0]), "index past the table")
    G.assert_same(G.bits(c[2]), G.bits(z[0]), "negative index")
    G.assert_same(G.bits(c[3:]), G.bits(a[3:]), "rows next to a bad index")


def _pm(rows, c, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.ones(rows, H)
    for r in range(rows):
        s[r, torch.randperm(H, generator=g)[:H // 2]] = -1.0
    return s * c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["closed", "open", "identity"])
def test_grn_exact(mode, dtype):
    rows = 37
    if mode == "identity":
        p = R.grn_params(31, dtype, gate=True)
        p["wg"] = torch.cat([torch.eye(H), torch.zeros(H, H)]).to(dtype)
        p["bg"] = torch.cat([torch.zeros(H), torch.full((H,), 40.0)])
        want_pre = _pm(rows, 2.0, 32)
        x = G.grid((rows, H), 33, dtype, "cpu")
        res = (want_pre - x.float()).to(dtype)
        kw = dict(res=res.to(DEV))
        c = 2.0
    else:
        p = R.grn_params(34, dtype)
        p["wg"] = torch.zeros(2 * H, H, dtype=dtype)
        c = 1.0 if mode == "closed" else 3.0
        x = _pm(rows, 1.0, 35).to(dtype)
        want_pre = x.float() * c
        p["bg"] = torch.cat([torch.zeros(H) if mode == "closed" else 2.0 * x[0].float(), torch.full((H,), -40.0 if mode == "closed" else 40.0)])
        if mode == "open":
            x = x[:1].expand(rows, H).contiguous()
            want_pre = x.float() * 3.0
        kw = {}
    p["gamma"], p["beta"] = torch.ones(H), torch.zeros(H)
    got = F.tft_grn_fwd(x.to(DEV), dev(p), **kw)
    want = (want_pre.double() / math.sqrt(c * c + 1e-3)).to(dtype)
    G.assert_same(G.bits(got.cpu()), G.bits(want), "exact GRN (%s)" % mode)


# ---- VSN ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvar", [1, 3, 4, 5])
def test_vsn_random(nvar, dtype):
    M = R.Mode("bar", dtype)
    for B, steps, ctx_on in ((1, 1, True), (3, 11, True), (4, 8, False), (5, 20, True)):      # 1, 33, 32 and 100 rows
        sd, a, b = R.vsn_params(nvar, 40 + nvar, dtype, ctx=ctx_on)
        pack = F.tft_vsn_pack(sd, a, b, dtype, DEV)
        T, t0 = steps + 3, 2
        g = torch.Generator().manual_seed(50 + B)
        split = [nvar] if nvar < 3 else [1, nvar - 2, 1]
        groups = [torch.randn(B, T, n, generator=g) for n in split]
        ctx = R.randn16((B, H), 60, dtype) if ctx_on else None
        out = G.Out((B, steps + 2, H), dtype, DEV, fill=torch.zeros(B, steps + 2, H))
        _, w = F.tft_vsn_fwd([t.to(DEV) for t in groups], pack, dtype, steps, t0=t0, ctx=ctx.to(DEV) if ctx_on else None, out=out.t, out_t0=1,
                             want_weights=True)
        x = torch.cat(groups, -1)[:, t0:t0 + steps].reshape(B * steps, nvar)
        ref, rw = R.vsn(M, x, R.vsn_nets({k: v for k, v in sd.items()}, "", M), a, b, R.V(ctx) if ctx_on else None, steps)
        got = out.check("tft_vsn_fwd")
        what = "vsn F %d rows %d ctx %d" % (nvar, B * steps, ctx_on)
        under_bar(got[:, 1:1 + steps].reshape(B * steps, H), ref, what)
        under_bar(w.reshape(B * steps, nvar), rw, what + " weights")
        assert float(got[:, 0].abs().max()) == 0 and float(got[:, steps + 1].abs().max()) == 0, "steps outside the window were written"
        assert float((w.double().sum(-1) - 1).abs().max()) <= (nvar + 2) * 2.0 ** -24
        if nvar == 1:
            assert torch.equal(w, torch.ones_like(w)), "one variable: the weight is exactly 1"
        no_w = F.tft_vsn_fwd([t.to(DEV) for t in groups], pack, dtype, steps, t0=t0, ctx=ctx.to(DEV) if ctx_on else None)
        G.assert_same(G.bits(no_w), G.bits(got[:, 1:1 + steps]), "with and without the weights output")


# ---- LSTM ---------------------------------------------------------------------------------------------------------------------------
def lstm_inputs(B, T, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xp = torch.randn(B, T, 4 * H, generator=g)
    whh = (torch.randn(4 * H, H, generator=g) / math.sqrt(H)).to(dtype)
    h0 = (0.5 * torch.randn(B, H, generator=g)).to(dtype)
    c0 = 0.5 * torch.randn(B, H, generator=g)
    return xp, whh, h0, c0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 5, 16, 17, 33])
def test_lstm_random(B, dtype):
    M = R.Mode("bar", dtype)
    for T in (1, 2, 9):
        xp, whh, h0, c0 = lstm_inputs(B, T, dtype, 70 + T)
        out, hn, cn = F.tft_lstm_fwd(xp.to(DEV), whh.to(DEV), h0.to(DEV), c0.to(DEV))
        hs, c = R.lstm(M, xp, whh.double(), R.V(h0), R.V(c0))
        for t in range(T):
            under_bar(out[:, t], hs[t], "lstm B %d T %d step %d" % (B, T, t))
        under_bar(cn, c, "lstm B %d T %d c" % (B, T))
        G.assert_same(G.bits(hn), G.bits(out[:, T - 1]), "hn")
        bars = [float(h.bar().mean()) for h in hs]
        assert bars[-1] >= bars[0], "the bar of the last step is not below the first step's"
        # c0 in 16 bits (what the static encoder hands over) equals the same values in fp32
        c16 = c0.to(dtype)
        a = F.tft_lstm_fwd(xp.to(DEV), whh.to(DEV), h0.to(DEV), c16.to(DEV))
        b = F.tft_lstm_fwd(xp.to(DEV), whh.to(DEV), h0.to(DEV), c16.float().to(DEV))
        G.assert_same(G.bits(a[0]), G.bits(b[0]), "c0 type")


@pytest.mark.parametrize("dtype", DTYPES)
def test_lstm_zero_recurrence_exact(dtype):
    """W_hh = 0; pre-activations in {-40, 0, 40}: sigmoid -> 0 (4e-18), 1/2, 1 and tanh -> -1, 0, 1 exactly, so with c0 on a k/4
    grid c_t = f c + i g is exact in fp32 as long as it stays on a grid: f, i in {0, 1/2, 1}, g in {-1, 0, 1}; h = o tanh(c) is
    checked where o = 0 (h = +-0 or 4e-18 tanh c -> rounds to 0) and through c itself."""
    B, T = 33, 9
    g = torch.Generator().manual_seed(81)
    pre = (torch.randint(-1, 2, (B, T, 4 * H), generator=g) * 40).float()
    pre[:, :, 3 * H:] = -40.0                                          # output gate closed: h = 0 every step, W_hh irrelevant anyway
    c0 = G.grid((B, H), 82, torch.float32, "cpu")
    whh = torch.zeros(4 * H, H, dtype=dtype)
    out, hn, cn = F.tft_lstm_fwd(pre.to(DEV), whh.to(DEV), torch.zeros(B, H, dtype=dtype, device=DEV), c0.to(DEV))
    c = c0.double()
    for t in range(T):
        i, f, gg = (pre[:, t, k * H:(k + 1) * H].double() for k in range(3))
        sg = lambda v: torch.where(v > 0, 1.0, torch.where(v < 0, 0.0, 0.5)).double()
        c = sg(f) * c + sg(i) * torch.sign(gg)
    # exp(-40) ~ 4e-18 instead of 0 in the closed gates: far below the fp32 spacing of any nonzero c on the 2^-(T+2) grid
    assert float((cn.double().cpu() - c).abs().max()) <= 1e-15 * 16
    assert float(out.float().abs().max()) < 1e-16


@pytest.mark.parametrize("dtype", DTYPES)
def test_lstm_handoff_and_row_alone(dtype):
    B, T = 33, 9
    xp, whh, h0, c0 = (t.to(DEV) for t in lstm_inputs(B, T, dtype, 90))
    out, hn, cn = F.tft_lstm_fwd(xp, whh, h0, c0)
    buf = torch.zeros(B, T, H, dtype=dtype, device=DEV)
    _, h6, c6 = F.tft_lstm_fwd(xp[:, :6], whh, h0, c0, out=buf[:, :6])
    _, h9, c9 = F.tft_lstm_fwd(xp[:, 6:], whh, h6, c6, out=buf[:, 6:])
    G.assert_same(G.bits(buf), G.bits(out), "6 + 3 steps against 9")
    G.assert_same(G.bits(h9), G.bits(hn), "hn after the hand-off")
    G.assert_same(G.bits(c9), G.bits(cn), "cn after the hand-off")
    for r in (0, 31, 32):
        o1, h1, c1 = F.tft_lstm_fwd(xp[r:r + 1].contiguous(), whh, h0[r:r + 1].contiguous(), c0[r:r + 1].contiguous())
        G.assert_same(G.bits(o1[0]), G.bits(out[r]), "row %d alone" % r)
        G.assert_same(G.bits(c1[0]), G.bits(cn[r]), "row %d alone, c" % r)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(12, 8), (40, 33), (192, 168)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=["T%d_enc%d" % s for s in SHAPES])
@pytest.mark.parametrize("B", [1, 3])
def test_attention_random(B, shape, dtype):
    T, enc = shape
    M = R.Mode("bar", dtype)
    for sigma in (1.0, 3.0):
        qkv = R.randn16((B * T, 288), 100 + T, dtype, sigma)
        wo = R.randn16((H, 32), 101, dtype, 1 / math.sqrt(32))
        out, probs = F.tft_attention_fwd(qkv.to(DEV), wo.to(DEV), B, T, enc, want_probs=True)
        ref, rp = R.attention(M, R.V(qkv), wo.double(), B, T, enc)
        under_bar(out, ref, "attention B %d T %d sigma %g" % (B, T, sigma))
        rp.e = rp.e + 1e-300                                       # (0 / 0 behind the mask)
        under_bar(probs, rp, "attention B %d T %d sigma %g probabilities" % (B, T, sigma))
        assert float((probs.double().sum(-1) - 1).abs().max()) <= (T + 8) * 2.0 ** -24
        behind = torch.arange(T)[None, :] > torch.arange(enc, T)[:, None]
        assert float(probs.cpu()[:, behind].abs().max()) == 0.0, "nonzero probability behind the mask"
        alone = F.tft_attention_fwd(qkv.to(DEV), wo.to(DEV), B, T, enc)
        G.assert_same(G.bits(alone), G.bits(out), "with and without the probabilities output")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=["T%d_enc%d" % s for s in SHAPES])
def test_attention_selector_exact(shape, dtype):
    """q = 32 e_0 in every head and k_j = 32 [j == j*] e_0: the score of key j* is 1024 / sqrt(32) = 181 above the others, whose
    fp32 exp(-181) is exactly 0 (the GAP of tests/_attention_reference.py is 104): P = one-hot(j*) exactly for every query at or after j*, so the
    output is round16(W_o round16(V_j*)) = W_o V_j* on k/4 grids (32 products, exact).  A query in front of j* (j* behind its mask)
    sees equal scores: the uniform mean over its keys, checked through the returned probabilities.  All key positions run in one
    batch: batch element b selects key b."""
    T, enc = shape
    B = T
    v = G.grid((B, T, 32), 111, dtype, "cpu", kmax=2)
    wo = G.grid((H, 32), 112, dtype, "cpu", kmax=2)
    qkv = torch.zeros(B, T, 288, dtype=dtype)
    for h in range(4):
        qkv[:, :, h * 32] = 32.0
        qkv[torch.arange(B), torch.arange(T), 128 + h * 32] = 32.0
    qkv[:, :, 256:] = v
    out, probs = F.tft_attention_fwd(qkv.reshape(B * T, 288).to(DEV), wo.to(DEV), B, T, enc, want_probs=True)
    out, probs = out.cpu(), probs.cpu()
    pos = torch.arange(enc, T)
    for b in range(B):
        seen = pos >= b                                               # queries that may see key b
        want = (v[b, b].double() @ wo.double().T).to(dtype)
        G.assert_same(G.bits(out[b, seen]), G.bits(want.expand(int(seen.sum()), H).contiguous()), "selected key %d" % b)
        onehot = torch.zeros(T)
        onehot[b] = 1.0
        assert torch.equal(probs[b, seen], onehot.expand(int(seen.sum()), T)), "probabilities of key %d" % b
        for qi in torch.nonzero(~seen).flatten().tolist():
            i = enc + qi
            want_p = torch.zeros(T)
            want_p[:i + 1] = torch.tensor(1.0) / torch.tensor(float(i + 1))
            assert torch.equal(probs[b, qi], want_p.float()), "key %d behind the mask of query %d" % (b, i)


# ---- argument checks: error codes, no launch -------------------------------------------------------------------------------------------
def test_argument_checks():
    dtype = HF
    x = R.randn16((4, H), 1, dtype).to(DEV)
    p = dev(R.grn_params(2, dtype))
    gate = dev(R.grn_params(3, dtype, gate=True))
    with pytest.raises(ValueError):
        F.tft_grn_fwd(x[:, :64], p)                                   # hidden size
    with pytest.raises(ValueError):
        F.tft_grn_fwd(x, gate)                                        # gate mode without a residual
    with pytest.raises(ValueError):
        F.tft_grn_fwd(x, p, ctx=x)                                    # no lin_c in this network
    lib = C.lib()
    out = G.Out((4, H), dtype, DEV)
    args = lambda xp, ldx, hidden: (xp, ldx, 0, 0, 0, 0, 1, 0, 0, 0, 0, C.ptr(p["wa"]), C.ptr(p["ba"]), 0, C.ptr(p["wi"]), C.ptr(p["bi"]),
                                    C.ptr(p["wg"]), C.ptr(p["bg"]), C.ptr(p["gamma"]), C.ptr(p["beta"]), 1e-3, C.ptr(out.t), H, 0, 0, 0, 0, 4,
                                    hidden, C.F16, C.stream())
    assert lib.dle_tft_grn_fwd(*args(0, H, H)) == -1                  # NULL
    assert lib.dle_tft_grn_fwd(*args(x.data_ptr() + 2, H, H)) == -1   # misaligned
    assert lib.dle_tft_grn_fwd(*args(x.data_ptr(), 64, H)) == -1      # pitch below the row
    assert lib.dle_tft_grn_fwd(*args(x.data_ptr(), H, 64)) == -1      # hidden size
    assert b"128" in lib.dle_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out.check("rejected tft_grn_fwd").float()).all(), "a rejected call wrote its output"
    qkv = R.randn16((2 * 12, 288), 5, dtype).to(DEV)
    wo = R.randn16((H, 32), 6, dtype).to(DEV)
    for bad in (dict(T=12, enc=12), dict(T=12, enc=0), dict(T=193, enc=8)):
        with pytest.raises(ValueError):
            F.tft_attention_fwd(qkv, wo, 2, bad["T"], bad["enc"])
    with pytest.raises(ValueError):
        F.tft_attention_fwd(qkv, wo, 2, 12, 8, heads=8)
    o = torch.empty(2, 4, H, dtype=dtype, device=DEV)
    assert lib.dle_tft_attention_fwd(qkv.data_ptr(), 288, wo.data_ptr(), o.data_ptr(), 0, 2, 12, 12, 4, 32, C.F16, C.stream()) == -1
    assert lib.dle_tft_attention_fwd(qkv.data_ptr(), 288, wo.data_ptr(), o.data_ptr(), 0, 2, 12, 8, 2, 64, C.F16, C.stream()) == -1
    assert lib.dle_tft_attention_fwd(qkv.data_ptr(), 280, wo.data_ptr(), o.data_ptr(), 0, 2, 12, 8, 4, 32, C.F16, C.stream()) == -1
    xp, whh, h0, c0 = (t.to(DEV) for t in lstm_inputs(2, 3, dtype, 7))
    with pytest.raises(ValueError):
        F.tft_lstm_fwd(xp[:, :, :256], whh, h0, c0)
    with pytest.raises(ValueError):
        F.tft_lstm_fwd(xp, whh, h0[:1], c0)
    assert lib.dle_tft_lstm_fwd(xp.data_ptr(), 3 * 512, 512, whh.data_ptr(), h0.data_ptr(), c0.data_ptr(), C.F32, 0, 0, 0, 0, 0, 2, 3, H,
                                C.F16, C.stream()) == -1              # no output at all
    assert lib.dle_tft_lstm_fwd(xp.data_ptr(), 3 * 512, 512, whh.data_ptr(), h0.data_ptr(), c0.data_ptr(), C.F32, 0, 0, 0, h0.data_ptr(), 0,
                                2, 3, 64, C.F16, C.stream()) == -1    # hidden size
    sd, a, b = R.vsn_params(9, 8, dtype)
    with pytest.raises(ValueError):
        F.tft_vsn_pack(sd, a, b, dtype, DEV)                          # more than 8 variables
    sd, a, b = R.vsn_params(2, 8, dtype)
    pack = F.tft_vsn_pack(sd, a, b, dtype, DEV)
    vals = torch.randn(2, 5, 2, device=DEV)
    ctx = R.randn16((2, H), 9, dtype).to(DEV)
    with pytest.raises(ValueError):
        F.tft_vsn_fwd([vals], pack, dtype, 6, ctx=ctx)                # window past the source steps
    with pytest.raises(ValueError):
        F.tft_vsn_fwd([vals[:, :, :1].contiguous()], pack, dtype, 5, ctx=ctx)   # column count
    with pytest.raises(ValueError):
        F.tft_vsn_fwd([vals], pack, dtype, 5)                         # the network has a lin_c: the context is required
    o = torch.empty(2, 5, H, dtype=dtype, device=DEV)
    vs = lambda n0, rows, t0: (vals.data_ptr(), 2, n0, 0, 0, 0, 0, 0, 0, 5, 5, t0, ctx.data_ptr(), H, C.ptr(pack["w16"]), C.ptr(pack["p32"]),
                               o.data_ptr(), H, 5, 0, 0, rows, H, 1e-3, C.F16, C.stream())
    assert lib.dle_tft_vsn_fwd(*vs(9, 10, 0)) == -1
    assert lib.dle_tft_vsn_fwd(*vs(2, 9, 0)) == -1                    # rows not a multiple of the steps
    assert lib.dle_tft_vsn_fwd(*vs(2, 10, 1)) == -1                   # window past the source
    assert lib.dle_tft_vsn_fwd(*vs(2, 10, 0)) == 0
    torch.cuda.synchronize()
