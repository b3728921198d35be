"""Float64 statement of the Temporal Fusion Transformer kernels (csrc/tft.hip) and of the whole forward pass, the emulated-rounding
variant of both, and per-element error bars obtained by running error analysis.  No GPU, no product kernel.

One code path, three modes (class Mode):
  exact   plain float64, nothing rounded: the function the kernels approximate;
  emul    float64 arithmetic, but every value is rounded to the 16-bit type exactly where the kernels / the forecaster round it
          (the project's yardstick: the best a kernel with these rounding points can do);
  bar     the exact values together with a per-element bar = e + 8 sigma.  e is a worst-case bound of the fp32 evaluation errors.
          sigma^2 is the variance of the accumulated 16-bit roundings, each taken as uniform over its rounding interval
          (variance ulp^2 / 12 = rnd^2 / 3) and independent of the others: through y = W x it becomes W^2 sigma^2 (a worst-case sum
          |W| rnd would grow by sum |W| ~ 9 per layer where the real error grows by ~1, and end 100 times above it after the
          three layers of a GRN); sums of two tracked values add their sigmas (they may be correlated: x and lin_a(x)), products
          and the nonlinear functions scale sigma by the magnitudes / Lipschitz constants below.  8 sigma: a Gaussian tail of
          1e-15 per element, with room for the correlation of errors that passed through a common matrix.  The rules for e:
            round to 16 bits      e' = e + rnd(|x| + e),  rnd(y) = max(2^-(m+1) y, half the subnormal spacing)   (m = 10 / 7)
            y = W x + b (fp32)    e' = (K + 2) u (|W||x| + |b|),  u = 2^-24: K products accumulated in fp32 in any order; the
                                  incoming e joins the variance as e^2 / 3 (an error bounded by e, taken as uniform), because
                                  |W| e would again grow ninefold per layer -- and per step of the LSTM
            ELU                   e' = e + 4 u |y|         (1-Lipschitz; expm1f within 4 ulp)
            sigmoid               e' = e / 4 + 8 u         (1/4-Lipschitz; __expf, the sum and the division)
            tanh                  e' = e + 8 u
            a * b                 e' = |a| e_b + |b| e_a + e_a e_b + u |a b|   (sigma^2: a^2 s_b + b^2 s_a + s_a s_b, the factors come
                                  from different rows of a matrix)
            a + b                 e' = e_a + e_b + u |a + b|
            LayerNorm             with d = x - mean, s = 1 / sqrt(var + eps), xh = d s:
                                  e' = |gamma| s (e + mean(e) + |xh| mean(|xh| e)) / (1 - 2 s max(bar)) + 6 u (|y - beta| + |beta|)
                                  first order in e; 1 / sqrt(var + eps) is 1-Lipschitz in the rms of the deviation, which gives
                                  the remainder factor; an ill-conditioned row (the joint LayerNorm over F nearly equal values)
                                  is capped at 2 sqrt(n) |gamma|, since |xh| <= sqrt(n) whatever the input; and the
                                  fp32 evaluation (two reductions of 128 terms contribute (128 + 2) u relative to sums that are
                                  themselves the quantities bounded; folded into the factor 6 u on the result and 130 u on the mean / variance)
            softmax               relative error of p_j <= t_j + sum_k p_k t_k + (n + 4) u,  t = e_s + (3 |s - max| + 20) u
Every bar is checked on the CPU (tests/test_tft_host.py): the emulated model stays below it, planted faults leave it.
"""
import math

import torch

U = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
EPS = 1e-3
H = 128
K_SIGMA = 8.0


class Mode:
    def __init__(self, kind, dtype=None):
        assert kind in ("exact", "emul", "bar")
        self.kind, self.dtype = kind, dtype
        self.round, self.track = kind == "emul", kind == "bar"


class V:
    """A float64 tensor with, in mode 'bar', a worst-case bound e of its fp32 evaluation error and the variance s of the
    accumulated 16-bit rounding errors."""
    __slots__ = ("v", "e", "s")

    def __init__(self, v, e=None, s=None):
        self.v = v.double()
        self.e = e if e is not None else torch.zeros_like(self.v)
        self.s = s if s is not None else torch.zeros_like(self.v)

    def __getitem__(self, idx):
        return V(self.v[idx], self.e[idx], self.s[idx])

    @property
    def sigma(self):
        return torch.sqrt(self.s)

    def bar(self):
        return self.e + K_SIGMA * self.sigma


def rnd(y, dtype):
    return torch.clamp(y * 2.0 ** -(MANT[dtype] + 1), min=2.0 ** (EMIN[dtype] - MANT[dtype] - 1))


def to16(x, dtype):
    return x.float().to(dtype).double()


def r16(M, a):
    if M.round:
        return V(to16(a.v, M.dtype))
    if M.track:
        return V(a.v, a.e, a.s + rnd(a.v.abs() + a.bar(), M.dtype) ** 2 / 3)
    return a


def w16(M, w):
    """A weight the product keeps in 16 bits."""
    return to16(w, M.dtype) if M.round else w.double()


def linear(M, a, W, b=None):
    W = W.double()
    v = a.v @ W.T
    if b is not None:
        v = v + b.double()
    if not M.track:
        return V(v)
    mag = a.v.abs() @ W.abs().T + (b.double().abs() if b is not None else 0.0)
    return V(v, (W.shape[1] + 2) * U * mag, (a.s + a.e ** 2 / 3) @ (W * W).T)


def add(M, a, b, indep=False):
    v = a.v + b.v
    if not M.track:
        return V(v)
    return V(v, a.e + b.e + U * v.abs(), a.s + b.s if indep else (a.sigma + b.sigma) ** 2)


def mul(M, a, b):
    v = a.v * b.v
    if not M.track:
        return V(v)
    return V(v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + U * v.abs(), a.v ** 2 * b.s + b.v ** 2 * a.s + a.s * b.s)


def elu(M, a):
    v = torch.where(a.v > 0, a.v, torch.expm1(a.v))
    return V(v, a.e + 4 * U * v.abs(), a.s) if M.track else V(v)


def sigmoid(M, a):
    return V(torch.sigmoid(a.v), a.e / 4 + 8 * U, a.s / 16) if M.track else V(torch.sigmoid(a.v))


def tanh(M, a):
    return V(torch.tanh(a.v), a.e + 8 * U, a.s) if M.track else V(torch.tanh(a.v))


def layernorm(M, a, gamma, beta, eps=EPS):
    gamma, beta = gamma.double(), beta.double()
    n = a.v.shape[-1]
    d = a.v - a.v.mean(-1, keepdim=True)
    s = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * s
    y = xh * gamma + beta
    if not M.track:
        return V(y)
    e = a.e + 130 * U * a.v.abs().mean(-1, keepdim=True)
    emax = (e + K_SIGMA * a.sigma).amax(-1, keepdim=True)
    rem = 1 / (1 - 2 * s * emax).clamp_min(1e-3)
    first = gamma.abs() * s * (e + e.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * e).mean(-1, keepdim=True) + 130 * U * xh.abs() / s)
    var = gamma ** 2 * s ** 2 * (a.s + 2.0 / n ** 2 * (a.s.sum(-1, keepdim=True) + xh ** 2 * (xh ** 2 * a.s).sum(-1, keepdim=True)))
    out = V(y, first * rem + 6 * U * ((y - beta).abs() + beta.abs()), var * rem ** 2)
    shrink = (2 * math.sqrt(n) * gamma.abs() / out.bar().clamp_min(1e-300)).clamp(max=1.0)      # |xh| <= sqrt(n) whatever the input
    return V(y, out.e * shrink, out.s * shrink ** 2)


def softmax(M, a, mask=None):
    """Softmax over the last axis; mask (bool) marks the allowed entries, the others are exactly zero."""
    s = a.v if mask is None else a.v.masked_fill(~mask, -math.inf)
    p = torch.softmax(s, -1)
    if not M.track:
        return V(p)
    t = a.e + (3 * (a.v - s.amax(-1, keepdim=True)).abs() + 20) * U
    sg = a.sigma
    if mask is not None:
        t, sg = t.masked_fill(~mask, 0.0), sg.masked_fill(~mask, 0.0)
    rel = t + (p * t).sum(-1, keepdim=True) + (a.v.shape[-1] + 4) * U
    return V(p, p * rel * 1.01, (p * (sg + (p * sg).sum(-1, keepdim=True)) * 1.01) ** 2)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
def grn(M, x, p, ctx=None, rows_per_ctx=1, res=None, wq=None, bq=None):
    """dle_tft_grn_fwd.  x (V) [rows, 128] holds 16-bit values; p: wa, ba, wc, wi, bi, wg, bg, gamma, beta (gate mode without wa).
    Returns (out rounded to 16 bits, quantile projection of the unrounded output or None)."""
    if "wa" in p:
        pre = linear(M, x, p["wa"], p["ba"])
        if ctx is not None:
            idx = torch.arange(x.v.shape[0]) // rows_per_ctx
            pre = add(M, pre, linear(M, ctx[idx], p["wc"]))
        g = r16(M, linear(M, r16(M, elu(M, pre)), p["wi"], p["bi"]))
        res = x
    else:
        g = x
    ab = linear(M, g, p["wg"], p["bg"])
    y = add(M, mul(M, ab[:, :H], sigmoid(M, ab[:, H:])), res)
    o = layernorm(M, y, p["gamma"], p["beta"])
    q = linear(M, o, wq, bq) if wq is not None else None
    return r16(M, o), q


def vsn(M, x, nets, a, b, ctx=None, rows_per_ctx=1):
    """dle_tft_vsn_fwd on raw values x [rows, F] (float64 of fp32 inputs).  nets: 'joint' (wa [128, F*128], ba, wc, wi, bi, wg
    [2F, 128], bg, wo [F, F*128], bo, gamma, beta [F]) and 'var' (a list of F GRN dicts); a, b [F, 128] the embedding.  The first
    linear of every network and the joint out_proj act on the unrounded embedding x_f a_f + b_f with unrounded weights (the kernel
    takes them folded; the fold's fp32 rounding and the F + 2 fused multiply-adds are (F + 4) u of the magnitudes).
    Returns (out rounded, weights [rows, F])."""
    F = x.shape[1]
    j = nets["joint"]
    emb = x.double().unsqueeze(-1) * a.double() + b.double()                   # [rows, F, 128]
    flat = emb.reshape(x.shape[0], F * H)

    def folded(W, bias):
        W, bias = W.double(), bias.double()
        v = flat @ W.T + bias
        if not M.track:
            return V(v)
        Wf = W.reshape(W.shape[0], F, H)
        mag = torch.einsum("rf,nf->rn", x.double().abs(), torch.einsum("nfh,fh->nf", Wf, a.double()).abs()) + \
            (torch.einsum("nfh,fh->n", Wf, b.double()) + bias).abs()
        return V(v, (F + 4) * U * mag)

    pre = folded(j["wa"], j["ba"])
    if ctx is not None:
        idx = torch.arange(x.shape[0]) // rows_per_ctx
        pre = add(M, pre, linear(M, ctx[idx], j["wc"]))
    g = r16(M, linear(M, r16(M, elu(M, pre)), j["wi"], j["bi"]))
    ab = linear(M, g, j["wg"], j["bg"])
    y = add(M, mul(M, ab[:, :F], sigmoid(M, ab[:, F:])), folded(j["wo"], j["bo"]))
    if F > 1:
        y = layernorm(M, y, j["gamma"], j["beta"])
    w = softmax(M, y)
    out = None
    for f in range(F):
        q = nets["var"][f]
        Wa, ba = q["wa"].double(), q["ba"].double()
        pre = V(emb[:, f] @ Wa.T + ba)
        if M.track:
            pre.e = 4 * U * (x[:, f:f + 1].double().abs() * (Wa @ a[f].double()).abs() + (Wa @ b[f].double() + ba).abs())
        g = r16(M, linear(M, r16(M, elu(M, pre)), q["wi"], q["bi"]))
        ab = linear(M, g, q["wg"], q["bg"])
        resid = V(emb[:, f], 2 * U * emb[:, f].abs() if M.track else None)
        o = layernorm(M, add(M, mul(M, ab[:, :H], sigmoid(M, ab[:, H:])), resid), q["gamma"], q["beta"])
        term = mul(M, V(w.v[:, f:f + 1].expand_as(o.v), w.e[:, f:f + 1].expand_as(o.v), w.s[:, f:f + 1].expand_as(o.v)), o)
        out = term if out is None else add(M, out, term)
    return r16(M, out), w


def lstm(M, xproj, whh, h0, c0, faults=()):
    """dle_tft_lstm_fwd: xproj [B, T, 512] (float64 of the fp32 input), whh [512, 128], h0 / c0 (V) [B, 128].  Returns the list of
    h per step (V, rounded), and the last c (V)."""
    h, c, hs = h0, c0, []
    for t in range(xproj.shape[1]):
        rec = linear(M, h, whh)
        gates = add(M, V(xproj[:, t].double()), rec)
        i, f, g, o = (gates[:, k * H:(k + 1) * H] for k in range(4))
        if "swap_gates" in faults:
            f, g = g, f
        c = add(M, mul(M, sigmoid(M, f), c), mul(M, sigmoid(M, i), tanh(M, g)), indep=True)
        h = r16(M, mul(M, sigmoid(M, o), tanh(M, c)))
        hs.append(h)
    return hs, c


def attention(M, qkv, wo, B, T, enc, n_head=4, faults=()):
    """dle_tft_attention_fwd: qkv (V) [B*T, (2 n_head + 1) d] 16-bit values, wo [128, d].  Returns (out (V) [B, T-enc, 128] rounded,
    mean probabilities (V) [B, T-enc, T])."""
    d = qkv.v.shape[1] // (2 * n_head + 1)
    scale = d ** -0.5
    x = qkv.v.reshape(B, T, -1)
    q = x[:, enc:, :n_head * d].reshape(B, T - enc, n_head, d).transpose(1, 2)
    k = x[:, :, n_head * d:2 * n_head * d].reshape(B, T, n_head, d).transpose(1, 2)
    v = x[:, :, 2 * n_head * d:]
    s = torch.matmul(q, k.transpose(2, 3)) * scale
    es = (d + 3) * U * scale * torch.matmul(q.abs(), k.abs().transpose(2, 3)) if M.track else None
    off = 1 if "mask_off_by_one" in faults else 0
    mask = (torch.arange(T)[None, :] <= (torch.arange(enc, T)[:, None] + off)).expand(B, n_head, T - enc, T)
    p = softmax(M, V(s, es), mask)
    pm = V(p.v.mean(1), p.e.mean(1) + 4 * U * p.v.mean(1), p.sigma.mean(1) ** 2) if M.track else V(p.v.mean(1))
    p16 = r16(M, pm)
    ctx = V(torch.matmul(p16.v, v), torch.matmul(p16.e, v.abs()) + (T + 2) * U * torch.matmul(p16.v, v.abs()),
            torch.matmul(p16.s, v * v)) if M.track else V(torch.matmul(p16.v, v))
    out = r16(M, linear(M, r16(M, ctx), wo))
    return out, pm


# ---- seeded parameters and inputs ----------------------------------------------------------------------------------------------------
def randn16(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def grn_params(seed, dtype, ctx=False, gate=False):
    """16-bit weights and fp32 vectors of one GRN (gate: GLU + LayerNorm only), scaled so that activations stay of order one."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    p = {"wg": (r(2 * H, H) / math.sqrt(H)).to(dtype), "bg": 0.1 * r(2 * H), "gamma": 1 + 0.1 * r(H), "beta": 0.1 * r(H)}
    if not gate:
        p.update(wa=(r(H, H) / math.sqrt(H)).to(dtype), ba=0.1 * r(H), wi=(r(H, H) / math.sqrt(H)).to(dtype), bi=0.1 * r(H))
        if ctx:
            p["wc"] = (r(H, H) / math.sqrt(H)).to(dtype)
    return p


def vsn_params(F, seed, dtype, ctx=True):
    """A selection network by the reference's parameter names (what functional.tft_vsn_pack takes) with 16-bit-representable
    matrices where the kernel keeps 16 bits, and its embedding [F, 128]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(dtype).float()
    sd = {"joint_grn.lin_a.weight": r(H, F * H) / math.sqrt(F * H), "joint_grn.lin_a.bias": 0.1 * r(H),
          "joint_grn.lin_i.weight": q(r(H, H) / math.sqrt(H)), "joint_grn.lin_i.bias": 0.1 * r(H),
          "joint_grn.glu.lin.weight": q(r(2 * F, H) / math.sqrt(H)), "joint_grn.glu.lin.bias": 0.1 * r(2 * F),
          "joint_grn.out_proj.weight": r(F, F * H) / math.sqrt(F * H), "joint_grn.out_proj.bias": 0.1 * r(F)}
    if ctx:
        sd["joint_grn.lin_c.weight"] = q(r(H, H) / math.sqrt(H))
    if F > 1:
        sd["joint_grn.layer_norm.ln.weight"], sd["joint_grn.layer_norm.ln.bias"] = 1 + 0.1 * r(F), 0.1 * r(F)
    for f in range(F):
        n = "var_grns.%d." % f
        sd.update({n + "lin_a.weight": r(H, H) / math.sqrt(H), n + "lin_a.bias": 0.1 * r(H),
                   n + "lin_i.weight": q(r(H, H) / math.sqrt(H)), n + "lin_i.bias": 0.1 * r(H),
                   n + "glu.lin.weight": q(r(2 * H, H) / math.sqrt(H)), n + "glu.lin.bias": 0.1 * r(2 * H),
                   n + "layer_norm.ln.weight": 1 + 0.1 * r(H), n + "layer_norm.ln.bias": 0.1 * r(H)})
    return sd, r(F, H), 0.1 * r(F, H)


def grn_of(sd, prefix, M, first_in_16=True):
    """One GRN of a state dict as the dictionary grn() / vsn() take; matrices the product keeps in 16 bits go through w16."""
    k = lambda n: sd[prefix + n]
    p = {"wa": w16(M, k("lin_a.weight")) if first_in_16 else k("lin_a.weight").double(), "ba": k("lin_a.bias").double(),
         "wi": w16(M, k("lin_i.weight")), "bi": k("lin_i.bias").double(), "wg": w16(M, k("glu.lin.weight")),
         "bg": k("glu.lin.bias").double()}
    if prefix + "lin_c.weight" in sd:
        p["wc"] = w16(M, k("lin_c.weight"))
    if prefix + "layer_norm.ln.weight" in sd:
        p["gamma"], p["beta"] = k("layer_norm.ln.weight").double(), k("layer_norm.ln.bias").double()
    if prefix + "out_proj.weight" in sd:
        p["wo"], p["bo"] = k("out_proj.weight").double(), k("out_proj.bias").double()
    return p


def vsn_nets(sd, prefix, M):
    F = sum(1 for k in sd if k.startswith(prefix + "var_grns.") and k.endswith("lin_a.bias"))
    return {"joint": grn_of(sd, prefix + "joint_grn.", M, first_in_16=False),
            "var": [grn_of(sd, prefix + "var_grns.%d." % f, M, first_in_16=False) for f in range(F)]}


def gate_of(sd, glu, ln, M):
    return {"wg": w16(M, sd[glu + ".lin.weight"]), "bg": sd[glu + ".lin.bias"].double(), "gamma": sd[ln + ".weight"].double(),
            "beta": sd[ln + ".bias"].double()}


# ---- the whole forward ----------------------------------------------------------------------------------------------------------------
def small_config(kind, T, enc, hidden=H):
    """'elec': one static categorical, three known, one target.  'obs': one observed continuous and two static continuous
    variables, two known, one target, no categorical."""
    from deeplearningexamples_amd.tft import model as TM
    feats = [TM.FeatureSpec("id", TM.InputTypes.ID, TM.DataTypes.CATEGORICAL), TM.FeatureSpec("t", TM.InputTypes.TIME, TM.DataTypes.CONTINUOUS),
             TM.FeatureSpec("y", TM.InputTypes.TARGET, TM.DataTypes.CONTINUOUS)]
    if kind == "elec":
        feats += [TM.FeatureSpec("k%d" % i, TM.InputTypes.KNOWN, TM.DataTypes.CONTINUOUS) for i in range(3)]
        feats += [TM.FeatureSpec("cat", TM.InputTypes.STATIC, TM.DataTypes.CATEGORICAL)]
        cats = [11]
    else:
        feats += [TM.FeatureSpec("k%d" % i, TM.InputTypes.KNOWN, TM.DataTypes.CONTINUOUS) for i in range(2)]
        feats += [TM.FeatureSpec("o0", TM.InputTypes.OBSERVED, TM.DataTypes.CONTINUOUS)]
        feats += [TM.FeatureSpec("s%d" % i, TM.InputTypes.STATIC, TM.DataTypes.CONTINUOUS) for i in range(2)]
        cats = []
    return TM.TFTConfig(features=feats, static_categorical_inp_lens=cats, example_length=T, encoder_length=enc, hidden_size=hidden)


def seeded_state(cfg, seed):
    """A state dict by the host model's names and shapes, filled from a seed: matrices ~ N(0, 1 / fan_in), embedding vectors and
    tables ~ N(0, 1), biases ~ 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1)."""
    from deeplearningexamples_amd.tft import model as TM
    ref = TM.TemporalFusionTransformer(cfg).state_dict()
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, t in ref.items():
        if name.endswith("_mask"):
            sd[name] = t.clone()
        elif "layer_norm" in name or name.endswith("_ln.weight") or name.endswith("_ln.bias"):
            sd[name] = (1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(t.shape, generator=g)
        elif "embedding_vectors" in name or "_embed." in name:
            sd[name] = torch.randn(t.shape, generator=g)
        elif t.dim() == 2 and "embedding_bias" not in name:
            sd[name] = torch.randn(t.shape, generator=g) / math.sqrt(t.shape[1])
        else:
            sd[name] = 0.1 * torch.randn(t.shape, generator=g)
    return sd


def seeded_batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    T = cfg.example_length
    rep = lambda t: t.unsqueeze(1).expand(B, T, t.shape[-1]).contiguous()
    b = {"s_cat": None, "s_cont": None, "k_cont": None, "o_cont": None, "target": torch.randn(B, T, 1, generator=g)}
    if cfg.static_categorical_inp_lens:
        b["s_cat"] = rep(torch.stack([torch.randint(0, n, (B,), generator=g) for n in cfg.static_categorical_inp_lens], -1))
    if cfg.static_continuous_inp_size:
        b["s_cont"] = rep(torch.randn(B, cfg.static_continuous_inp_size, generator=g))
    if cfg.temporal_known_continuous_inp_size:
        b["k_cont"] = torch.randn(B, T, cfg.temporal_known_continuous_inp_size, generator=g)
    if cfg.temporal_observed_continuous_inp_size:
        b["o_cont"] = torch.randn(B, T, cfg.temporal_observed_continuous_inp_size, generator=g)
    return b


def forward(M, sd, cfg, batch):
    """The forecaster's chain (tft/infer.py) in mode M -> dict(out [B, T-enc, Q], hist_w, fut_w, probs), float64 tensors."""
    assert not M.track
    B, T, enc = batch["target"].shape[0], cfg.example_length, cfg.encoder_length
    e = "embedding."
    P = "TFTpart2."
    # static path
    if cfg.num_static_vars == 1 and cfg.static_categorical_inp_lens:
        rows = V(w16(M, sd[e + "s_cat_embed.0.weight"])[batch["s_cat"][:, 0, 0]])
        p = grn_of(sd, "static_encoder.vsn.var_grns.0.", M)
        sctx, _ = grn(M, rows, p)
    else:
        assert not cfg.static_categorical_inp_lens
        sctx, _ = vsn(M, batch["s_cont"][:, 0].double(), vsn_nets({k: v for k, v in sd.items() if "static_encoder.vsn.joint_grn.lin_c" not in k},
                                                                  "static_encoder.vsn.", M),
                      sd[e + "s_cont_embedding_vectors"], sd[e + "s_cont_embedding_bias"])
    cs, ce, ch, cc = (grn(M, sctx, grn_of(sd, "static_encoder.context_grns.%d." % i, M))[0] for i in range(4))
    # temporal selection
    cols, av, bv = [], [], []
    for key, name in (("o_cont", "t_cont_o"), ("k_cont", "t_cont_k"), ("target", "t_tgt")):
        if batch.get(key) is not None:
            cols.append(batch[key].double())
            av.append(sd[e + name + "_embedding_vectors"])
            bv.append(sd[e + name + "_embedding_bias"])
    hist_x = torch.cat(cols, -1)[:, :enc].reshape(B * enc, -1)
    hist, hist_w = vsn(M, hist_x, vsn_nets(sd, P + "history_vsn.", M), torch.cat(av), torch.cat(bv), cs, enc)
    fut_x = batch["k_cont"].double()[:, enc:].reshape(B * (T - enc), -1)
    fut, fut_w = vsn(M, fut_x, vsn_nets(sd, P + "future_vsn.", M), sd[e + "t_cont_k_embedding_vectors"], sd[e + "t_cont_k_embedding_bias"],
                     cs, T - enc)
    feat = torch.cat([hist.v.reshape(B, enc, H), fut.v.reshape(B, T - enc, H)], 1)
    # the two LSTMs, the future one from the history one's state
    def proj(x, name):
        n = P + name
        return x @ w16(M, sd[n + ".weight_ih_l0"]).T + (sd[n + ".bias_ih_l0"].double() + sd[n + ".bias_hh_l0"].double())
    hs1, c1 = lstm(M, proj(feat[:, :enc], "history_encoder"), w16(M, sd[P + "history_encoder.weight_hh_l0"]), ch, cc)
    hs2, _ = lstm(M, proj(feat[:, enc:], "future_encoder"), w16(M, sd[P + "future_encoder.weight_hh_l0"]), hs1[-1], c1)
    seq = torch.stack([h.v for h in hs1 + hs2], 1).reshape(B * T, H)
    temporal, _ = grn(M, V(seq), gate_of(sd, P + "input_gate", P + "input_gate_ln", M), res=V(feat.reshape(B * T, H)))
    enriched, _ = grn(M, temporal, grn_of(sd, P + "enrichment_grn.", M), ctx=ce, rows_per_ctx=T)
    qkv = r16(M, V(enriched.v @ w16(M, sd[P + "attention.qkv_linears.weight"]).T))
    att, probs = attention(M, qkv, w16(M, sd[P + "attention.out_proj.weight"]), B, T, enc, cfg.n_head)
    tail = lambda a: V(a.v.reshape(B, T, H)[:, enc:].reshape(B * (T - enc), H))
    x, _ = grn(M, V(att.v.reshape(B * (T - enc), H)), gate_of(sd, P + "attention_gate", P + "attention_ln", M), res=tail(enriched))
    x, _ = grn(M, x, grn_of(sd, P + "positionwise_grn.", M))
    _, q = grn(M, x, gate_of(sd, P + "decoder_gate", P + "decoder_ln", M), res=tail(temporal),
               wq=sd[P + "quantile_proj.weight"], bq=sd[P + "quantile_proj.bias"])
    return {"out": q.v.reshape(B, T - enc, -1), "hist_w": hist_w.v.reshape(B, enc, -1), "fut_w": fut_w.v.reshape(B, T - enc, -1),
            "probs": probs.v}


def host_forward(sd, cfg, batch):
    """The host model (torch operators, float64) on the same state and batch: what forward(Mode('exact')) must reproduce."""
    from deeplearningexamples_amd.tft import model as TM
    m = TM.TemporalFusionTransformer(cfg).double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    with torch.no_grad():
        return m.eval()({k: (v.double() if v is not None and v.is_floating_point() else v) for k, v in batch.items()})


class Scaler:
    """Stand-in for the scalers the reference pickles (sklearn's StandardScaler): the command-line test pickles this class."""

    def __init__(self, mean, scale):
        self.mean, self.scale = float(mean), float(scale)

    def inverse_transform(self, x):
        return x * self.scale + self.mean
