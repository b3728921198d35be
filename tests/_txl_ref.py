"""Float64 restatement of the Transformer-XL evaluation model (helpers only; no tests here).

`RefModel.forward` follows LanguageModeling/Transformer-XL/pytorch/mem_transformer.py for attn_type 0, post-LayerNorm: the memory
holds HIDDEN states, K and V of the whole window are recomputed in every segment, `pos_emb` and `r_net(pos_emb)` are rebuilt per
segment, BD goes through the pad / view / narrow `_rel_shift`, the masks are the triu / tril sums of `_forward`, and the loss is
ProjectedAdaptiveLogSoftmax with keep_order (utils/proj_adaptive_softmax.py:131-208).  tests/test_txl_host.py pins it to the
reference's own float64 output.

`RefModel.forward_kv` is the formulation the evaluator runs: K / V rows are cached, `r` is a table indexed by distance, the mask
is the band `(i - shift < j) and (j <= i + mlen)`.  With `dtype` set it rounds to that 16-bit type wherever the evaluator does
(the emulated variant); with `dtype=None` it is float64 throughout and must equal `forward`.

Weights come from `fill_state(cfg, seed)`: an integer hash of (tensor, element, seed), so they are regenerated, never stored.
"""
import math

import numpy as np
import torch

F64 = torch.float64


def small_config(div_val=1, same_length=False, clamp_len=-1, tgt_len=8, mem_len=20):
    """MemTransformerLM keyword arguments of the small test model."""
    return {
        "n_token": 1000, "n_layer": 2, "n_head": 2, "d_model": 128, "d_head": 64, "d_inner": 256, "dropout": 0.0, "dropatt": 0.0,
        "dtype": None, "tie_weight": True, "d_embed": 128, "div_val": div_val, "tie_projs": [False, True, True, True],
        "pre_lnorm": False, "tgt_len": tgt_len, "ext_len": 0, "mem_len": mem_len, "cutoffs": [100, 300, 600],
        "same_length": same_length, "attn_type": 0, "clamp_len": clamp_len, "sample_softmax": -1,
    }


# the cases of the golden file: (name, div_val, same_length, clamp_len)
CASES = [("dv1", 1, False, -1), ("dv2", 2, False, -1), ("dv1_same", 1, True, -1), ("dv1_clamp", 1, False, 12),
         ("dv2_same_clamp", 2, True, 12)]
SEGMENTS = [8, 8, 8, 8, 8, 3]      # five segments of tgt_len 8 and a short last one
BATCH = 3


def state_shapes(cfg):
    """name -> shape of MemTransformerLM(**cfg).state_dict() (tests/golden/txl_state_dict.json pins this list for base / large)."""
    n_token, d_model, d_embed, div_val = cfg["n_token"], cfg["d_model"], cfg["d_embed"], cfg["div_val"]
    h = cfg["n_head"] * cfg["d_head"]
    ends = [0] + list(cfg["cutoffs"]) + [n_token]
    ncl = len(ends) - 1
    out = {}
    if div_val == 1:
        out["word_emb.emb_layers.0.weight"] = (n_token, d_embed)
        if d_model != d_embed:
            out["word_emb.emb_projs.0"] = (d_model, d_embed)
    else:
        for i in range(ncl):
            out["word_emb.emb_layers.%d.weight" % i] = (ends[i + 1] - ends[i], d_embed // div_val ** i)
            out["word_emb.emb_projs.%d" % i] = (d_model, d_embed // div_val ** i)
    for l in range(cfg["n_layer"]):
        p = "layers.%d." % l
        out[p + "dec_attn.qkv_net.weight"] = (3 * h, d_model)
        out[p + "dec_attn.o_net.weight"] = (d_model, h)
        out[p + "dec_attn.layer_norm.weight"] = (d_model,)
        out[p + "dec_attn.layer_norm.bias"] = (d_model,)
        out[p + "dec_attn.r_net.weight"] = (h, d_model)
        out[p + "pos_ff.CoreNet.0.weight"] = (cfg["d_inner"], d_model)
        out[p + "pos_ff.CoreNet.0.bias"] = (cfg["d_inner"],)
        out[p + "pos_ff.CoreNet.3.weight"] = (d_model, cfg["d_inner"])
        out[p + "pos_ff.CoreNet.3.bias"] = (d_model,)
        out[p + "pos_ff.layer_norm.weight"] = (d_model,)
        out[p + "pos_ff.layer_norm.bias"] = (d_model,)
    if ncl > 1:
        out["crit.cluster_weight"] = (ncl - 1, d_embed)
        out["crit.cluster_bias"] = (ncl - 1,)
    tied_w = cfg["tie_weight"]
    if div_val == 1:
        out["crit.out_layers_biases.0"] = (n_token,)
        if not tied_w:
            out["crit.out_layers_weights.0"] = (n_token, d_embed)
        if d_model != d_embed:
            for i in range(ncl):
                if not cfg["tie_projs"][i]:
                    out["crit.out_projs.%d" % i] = (d_model, d_embed)
            out["crit.shared_out_projs.0"] = (d_model, d_embed)
    else:
        for i in range(ncl):
            out["crit.out_layers_biases.%d" % i] = (ends[i + 1] - ends[i],)
            if not tied_w:
                out["crit.out_layers_weights.%d" % i] = (ends[i + 1] - ends[i], d_embed // div_val ** i)
            if not cfg["tie_projs"][i]:
                out["crit.out_projs.%d" % i] = (d_model, d_embed // div_val ** i)
            out["crit.shared_out_projs.%d" % i] = (d_model, d_embed // div_val ** i)
    out["pos_emb.inv_freq"] = (d_model // 2,)
    out["r_w_bias"] = (cfg["n_head"], cfg["d_head"])
    out["r_r_bias"] = (cfg["n_head"], cfg["d_head"])
    return out


def _hash_uniform(n, salt):
    """n values in [-0.5, 0.5) from integer arithmetic only (the same on every platform and library version)."""
    k = np.arange(n, dtype=np.uint64)
    x = (k + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return (x >> np.uint64(40)).astype(np.float64) / float(1 << 24) - 0.5


def fill_state(cfg, seed):
    """A float64 state dict with the reference's names; tied entries (crit.shared_out_projs.*) alias word_emb.emb_projs.*."""
    state = {}
    for idx, (name, shape) in enumerate(sorted(state_shapes(cfg).items())):
        if name.startswith("crit.shared_out_projs."):
            continue
        n = int(np.prod(shape))
        u = torch.from_numpy(_hash_uniform(n, (seed * 1000 + idx) * 1000003)).reshape(shape)
        if name == "pos_emb.inv_freq":
            d = cfg["d_model"]
            state[name] = 1.0 / (10000 ** (torch.arange(0.0, d, 2.0, dtype=F64) / d))
        elif name.endswith("layer_norm.weight"):
            state[name] = 1.0 + 0.2 * u
        elif name.endswith("bias") or ".out_layers_biases." in name:
            state[name] = 0.2 * u
        elif name.startswith("word_emb.emb_layers"):
            state[name] = 0.3 * u
        elif len(shape) == 2:
            state[name] = u * (3.0 / math.sqrt(shape[1]))
        else:
            state[name] = 0.2 * u
    for name in state_shapes(cfg):
        if name.startswith("crit.shared_out_projs."):
            state[name] = state["word_emb.emb_projs." + name.rsplit(".", 1)[1]]
    return state


def make_tokens(cfg, seed, n):
    """n token ids that visit the shortlist and every cluster (integer hash, as the weights)."""
    u = _hash_uniform(n, seed * 7919 + 17) + 0.5
    ends = [0] + list(cfg["cutoffs"]) + [cfg["n_token"]]
    which = (_hash_uniform(n, seed * 104729 + 5) + 0.5) * (len(ends) - 1)
    lo = np.array(ends)[which.astype(np.int64)]
    hi = np.array(ends)[which.astype(np.int64) + 1]
    return torch.from_numpy((lo + u * (hi - lo)).astype(np.int64))


def stream_batches(tokens, bsz, segments):
    """[(data [q, bsz], target [q, bsz])] of an ordered stream laid out as LMOrderedIterator does, segment lengths given."""
    n_step = tokens.numel() // bsz
    data = tokens[:n_step * bsz].view(bsz, -1).t().contiguous()
    out, i = [], 0
    for q in segments:
        out.append((data[i:i + q], data[i + 1:i + 1 + q]))
        i += q
    assert i + 1 <= data.shape[0]
    return out


def rel_shift(x):
    """RelMultiHeadAttn._rel_shift: the pad / view / narrow trick on [B, N, qlen, klen]."""
    zero_pad = torch.zeros((x.size(0), x.size(1), x.size(2), 1), dtype=x.dtype)
    x_padded = torch.cat([zero_pad, x], dim=3)
    x_padded = x_padded.view(x.size(0), x.size(1), x.size(3) + 1, x.size(2))
    return x_padded.narrow(2, 1, x_padded.size(2) - 1).view_as(x)


def band_shift(cfg, qlen, klen):
    """`shift` of allowed(i, j) = (i - shift < j) and (j <= i + mlen): the same_length mask of _forward, else no lower bound."""
    if cfg["same_length"]:
        mask_len = klen - cfg["mem_len"] - 1
        return qlen - mask_len if mask_len > 0 else qlen
    return qlen


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


class RefModel:
    def __init__(self, cfg, state):
        self.cfg = cfg
        self.s = {k: v.to(F64) for k, v in state.items()}
        self.ends = [0] + list(cfg["cutoffs"]) + [cfg["n_token"]]
        self.ncl = len(self.ends) - 1
        self.H = cfg["n_head"] * cfg["d_head"]

    # ---- rounding: identity in float64 mode, once-to-16-bit in the emulated mode
    @staticmethod
    def _r(x, dtype):
        return x if dtype is None else x.to(dtype).to(F64)

    # ---- adaptive embedding (mem_transformer.py:484-513)
    def embed(self, inp, dtype=None):
        cfg, s, r = self.cfg, self.s, self._r
        scale = cfg["d_model"] ** 0.5
        flat = inp.reshape(-1)
        if cfg["div_val"] == 1:
            e = r(s["word_emb.emb_layers.0.weight"], dtype)[flat]
            if cfg["d_model"] != cfg["d_embed"]:
                e = r(e @ r(s["word_emb.emb_projs.0"], dtype).t(), dtype)
            return r(e * (float(np.float32(scale)) if dtype is not None else scale), dtype).view(*inp.shape, -1)
        out = torch.zeros(flat.numel(), cfg["d_model"], dtype=F64)
        for i in range(self.ncl):
            lo, hi = self.ends[i], self.ends[i + 1]
            idx = ((flat >= lo) & (flat < hi)).nonzero().reshape(-1)
            if idx.numel() == 0:
                continue
            e = r(s["word_emb.emb_layers.%d.weight" % i], dtype)[flat[idx] - lo]
            e = r(e @ r(s["word_emb.emb_projs.%d" % i], dtype).t(), dtype)
            out[idx] = r(e * (float(np.float32(scale)) if dtype is not None else scale), dtype)
        return out.view(*inp.shape, -1)

    # ---- adaptive softmax with keep_order (proj_adaptive_softmax.py:131-208)
    def _out_weight(self, i):
        s, cfg = self.s, self.cfg
        if cfg["div_val"] == 1:
            w = s["word_emb.emb_layers.0.weight"] if cfg["tie_weight"] else s["crit.out_layers_weights.0"]
            return w[self.ends[i]:self.ends[i + 1]], s["crit.out_layers_biases.0"][self.ends[i]:self.ends[i + 1]]
        w = s["word_emb.emb_layers.%d.weight" % i] if cfg["tie_weight"] else s["crit.out_layers_weights.%d" % i]
        return w, s["crit.out_layers_biases.%d" % i]

    def _out_proj(self, i):
        s, cfg = self.s, self.cfg
        if cfg["tie_projs"][i]:
            if cfg["div_val"] == 1:
                return s.get("word_emb.emb_projs.0")
            return s["word_emb.emb_projs.%d" % i]
        return s.get("crit.out_projs.%d" % i)

    def _logit(self, hidden, w, b, proj, dtype):
        r = self._r
        if proj is not None:
            hidden = r(hidden @ r(proj, dtype), dtype)
        x = hidden @ r(w, dtype).t() + b
        return x if dtype is None else x.to(torch.float32).to(F64)

    def nll(self, hidden, target, dtype=None):
        w0, b0 = self._out_weight(0)
        if self.ncl > 1:
            w0 = torch.cat([w0, self.s["crit.cluster_weight"]], 0)
            b0 = torch.cat([b0, self.s["crit.cluster_bias"]], 0)
        head = torch.log_softmax(self._logit(hidden, w0, b0, self._out_proj(0), dtype), dim=1)
        out = torch.zeros(target.numel(), dtype=F64)
        for i in range(self.ncl):
            lo, hi = self.ends[i], self.ends[i + 1]
            idx = ((target >= lo) & (target < hi)).nonzero().reshape(-1)
            if idx.numel() == 0:
                continue
            t = target[idx] - lo
            if i == 0:
                lp = head[idx].gather(1, t[:, None]).squeeze(1)
            else:
                w, b = self._out_weight(i)
                tail = torch.log_softmax(self._logit(hidden[idx], w, b, self._out_proj(i), dtype), dim=1)
                lp = head[idx][:, -i] + tail.gather(1, t[:, None]).squeeze(1)
            out[idx] = -lp
        return out

    # ---- the reference's formulation: hidden-state memory, everything recomputed per segment
    def forward(self, data, target, mems):
        cfg, s = self.cfg, self.s
        qlen, bsz = data.shape
        nh, dh = cfg["n_head"], cfg["d_head"]
        x = self.embed(data)
        mlen = mems[0].shape[0] if mems is not None else 0
        klen = mlen + qlen
        ones = torch.ones(qlen, klen, dtype=F64)
        if cfg["same_length"]:
            mask_len = klen - cfg["mem_len"] - 1
            msl = qlen - mask_len if mask_len > 0 else qlen
            mask = (torch.triu(ones, 1 + mlen) + torch.tril(ones, -msl)).bool()
        else:
            mask = torch.triu(ones, diagonal=1 + mlen).bool()
        pos_seq = torch.arange(klen - 1, -1, -1.0, dtype=F64)
        if cfg["clamp_len"] > 0:
            pos_seq = pos_seq.clamp(max=cfg["clamp_len"])
        sin_inp = torch.outer(pos_seq, s["pos_emb.inv_freq"])
        pos_emb = torch.cat([sin_inp.sin(), sin_inp.cos()], dim=-1)
        hids = []
        for l in range(cfg["n_layer"]):
            p = "layers.%d." % l
            hids.append(x)
            cat = torch.cat([mems[l], x], 0) if (mems is not None and mems[l].shape[0]) else x
            heads = cat @ s[p + "dec_attn.qkv_net.weight"].t()
            r_k = (pos_emb @ s[p + "dec_attn.r_net.weight"].t()).view(klen, nh, dh)
            q, k, v = torch.chunk(heads, 3, dim=-1)
            q = q[-qlen:].reshape(qlen, bsz, nh, dh)
            k = k.reshape(klen, bsz, nh, dh)
            v = v.reshape(klen, bsz, nh, dh)
            ac = torch.einsum("ibnd,jbnd->bnij", q + s["r_w_bias"], k)
            bd = rel_shift(torch.einsum("ibnd,jnd->bnij", q + s["r_r_bias"], r_k))
            score = (ac + bd) * (1.0 / dh ** 0.5)
            score = score.masked_fill(mask[None, None], -float("inf"))
            prob = torch.softmax(score, dim=3)
            vec = torch.einsum("bnij,jbnd->ibnd", prob, v).reshape(qlen, bsz, nh * dh)
            x = layer_norm(x + vec @ s[p + "dec_attn.o_net.weight"].t(), s[p + "dec_attn.layer_norm.weight"],
                           s[p + "dec_attn.layer_norm.bias"])
            ff = torch.relu(x @ s[p + "pos_ff.CoreNet.0.weight"].t() + s[p + "pos_ff.CoreNet.0.bias"])
            ff = ff @ s[p + "pos_ff.CoreNet.3.weight"].t() + s[p + "pos_ff.CoreNet.3.bias"]
            x = layer_norm(x + ff, s[p + "pos_ff.layer_norm.weight"], s[p + "pos_ff.layer_norm.bias"])
        # _update_mems for ext_len == 0
        if cfg["mem_len"] > 0:
            end = mlen + qlen
            beg = max(0, end - cfg["mem_len"])
            new = [(torch.cat([mems[l], hids[l]], 0) if (mems is not None and mems[l].shape[0]) else hids[l])[beg:end]
                   for l in range(cfg["n_layer"])]
        else:
            new = None
        loss = self.nll(x.reshape(-1, x.shape[-1]), target.reshape(-1)).view(qlen, bsz)
        return loss, new

    # ---- the evaluator's formulation: cached K / V, r by distance, band mask; dtype = the emulated 16-bit variant
    def dist_table(self, l, n_dist, dtype=None):
        cfg, s, r = self.cfg, self.s, self._r
        d = torch.arange(n_dist, dtype=F64)
        if cfg["clamp_len"] > 0:
            d = d.clamp(max=cfg["clamp_len"])
        sin_inp = torch.outer(d, s["pos_emb.inv_freq"])
        pos = r(torch.cat([sin_inp.sin(), sin_inp.cos()], dim=-1), dtype)
        return r(pos @ r(s["layers.%d.dec_attn.r_net.weight" % l], dtype).t(), dtype)

    def forward_kv(self, data, target, cache, dtype=None):
        """cache: None or a list per layer of (K [mlen, bsz, H], V [mlen, bsz, H]) -> (loss [qlen, bsz], new cache)."""
        cfg, s, r = self.cfg, self.s, self._r
        qlen, bsz = data.shape
        nh, dh, H = cfg["n_head"], cfg["d_head"], self.H
        x = self.embed(data, dtype)
        mlen = cache[0][0].shape[0] if cache is not None else 0
        klen = mlen + qlen
        shift = band_shift(cfg, qlen, klen)
        i = torch.arange(qlen)[:, None]
        j = torch.arange(klen)[None, :]
        allowed = (i - shift < j) & (j <= i + mlen)
        dist = (i + mlen - j).clamp(min=0)
        new = []
        for l in range(cfg["n_layer"]):
            p = "layers.%d." % l
            qkv = r(x @ r(s[p + "dec_attn.qkv_net.weight"], dtype).t(), dtype)
            q, k, v = torch.chunk(qkv, 3, dim=-1)
            if cache is not None and mlen:
                k = torch.cat([cache[l][0], k], 0)
                v = torch.cat([cache[l][1], v], 0)
            beg = max(0, klen - cfg["mem_len"])
            new.append((k[beg:klen], v[beg:klen]) if cfg["mem_len"] > 0 else (k[:0], v[:0]))
            table = self.dist_table(l, klen, dtype).view(klen, nh, dh)
            q4 = q.reshape(qlen, bsz, nh, dh)
            a = r(q4 + r(s["r_w_bias"], dtype), dtype)
            b = r(q4 + r(s["r_r_bias"], dtype), dtype)
            ac = torch.einsum("ibnd,jbnd->bnij", a, k.reshape(klen, bsz, nh, dh))
            g = torch.einsum("ibnd,end->bnie", b, table)                      # by distance
            bd = g.gather(3, dist[None, None].expand(bsz, nh, qlen, klen))
            scale = 1.0 / dh ** 0.5
            score = ((ac + bd) * scale).masked_fill(~allowed[None, None], -float("inf"))
            if dtype is None:
                prob = torch.softmax(score, dim=3)
            else:
                e = torch.exp(score - score.max(dim=3, keepdim=True).values)
                prob = r(e, dtype) / e.sum(dim=3, keepdim=True)
            vec = r(torch.einsum("bnij,jbnd->ibnd", prob, v.reshape(klen, bsz, nh, dh)).reshape(qlen, bsz, H), dtype)
            o = r(vec @ r(s[p + "dec_attn.o_net.weight"], dtype).t(), dtype)
            x = r(layer_norm(r(x + o, dtype), s[p + "dec_attn.layer_norm.weight"], s[p + "dec_attn.layer_norm.bias"]), dtype)
            ff = r(torch.relu(x @ r(s[p + "pos_ff.CoreNet.0.weight"], dtype).t() + s[p + "pos_ff.CoreNet.0.bias"]), dtype)
            ff = r(ff @ r(s[p + "pos_ff.CoreNet.3.weight"], dtype).t() + s[p + "pos_ff.CoreNet.3.bias"], dtype)
            x = r(layer_norm(r(x + ff, dtype), s[p + "pos_ff.layer_norm.weight"], s[p + "pos_ff.layer_norm.bias"]), dtype)
        loss = self.nll(x.reshape(-1, x.shape[-1]), target.reshape(-1), dtype).view(qlen, bsz)
        return loss, new

    def run(self, batches, how="forward", dtype=None):
        """Losses per segment over a stream of (data, target), memory carried along; also the final memory / cache."""
        state, out = None, []
        for data, target in batches:
            if how == "forward":
                loss, state = self.forward(data, target, state)
            else:
                loss, state = self.forward_kv(data, target, state, dtype)
            out.append(loss)
        return out, state


# ================================================================================================ the attention kernel alone
# dle_txl_rel_attention_fwd (include/dle_mi355x.h): float64 statement, per-element bar, and an fp32 model of the kernel's arithmetic.
U32 = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
TILE = 32                       # queries per workgroup = keys per tile; a wavefront takes every fourth tile of the band
ATTN_FAULTS = ("skew_off_by_one", "upper_edge", "lower_edge", "stale_max", "ring_start")


def attn_inputs(B, nh, qlen, mlen, dtype, seed, sigma=1.0):
    """Seeded N(0, sigma) queries and N(0, 1) keys / values / table in `dtype`: q is the first third of a [B*qlen, 3H] buffer."""
    g = torch.Generator().manual_seed(seed)
    H, klen = nh * 64, mlen + qlen
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    qkv = (sigma * n(B * qlen, 3 * H)).to(dtype)
    return dict(B=B, nh=nh, qlen=qlen, mlen=mlen, klen=klen, H=H, dtype=dtype, qkv=qkv, u=(0.5 * n(nh, 64)).to(dtype),
                v=(0.5 * n(nh, 64)).to(dtype), K=n(B, klen, H).to(dtype), V=n(B, klen, H).to(dtype), r=n(klen + 5, H).to(dtype))


def ring_of(K, V, cap, start, fill):
    """Physical ring [B, cap, 2H] holding logical row j at (start + j) % cap and `fill` in every other row."""
    B, klen, H = K.shape
    kv = torch.full((B, cap, 2 * H), fill, dtype=K.dtype)
    phys = (start + torch.arange(klen)) % cap
    kv[:, phys, :H] = K
    kv[:, phys, H:] = V
    return kv


def ring_configs(qlen, mlen):
    """(cap, start): tight (cap = klen, the window wraps) and slack (cap = klen + 37, the wrap falls inside a key tile)."""
    klen = qlen + mlen
    tight = (klen, (klen // 2 + 1) % klen)
    cap = klen + 37
    return [tight, (cap, cap - min(klen - 1, 13) if klen > 1 else cap - 1)]


def shift_choices(qlen):
    return [1 << 30, 1, max(1, qlen - 3)]


def allowed_mask(qlen, mlen, shift):
    i = torch.arange(qlen)[:, None]
    j = torch.arange(qlen + mlen)[None, :]
    return (i - shift < j) & (j <= i + mlen)


def spec_ab(inp):
    """a = round16(float(q) + float(u)), b = round16(float(q) + float(v)) with fp32 sums: part of the function's definition."""
    B, nh, qlen, H, dt = inp["B"], inp["nh"], inp["qlen"], inp["H"], inp["dtype"]
    q = inp["qkv"][:, :H].float().view(B, qlen, nh, 64)
    return (q + inp["u"].float()).to(dt), (q + inp["v"].float()).to(dt)


def attn_reference(inp, shift, scale):
    """float64: ctx [B, nh, qlen, 64] and what the bar needs (scores, probabilities, magnitudes)."""
    B, nh, qlen, mlen, klen = inp["B"], inp["nh"], inp["qlen"], inp["mlen"], inp["klen"]
    a, b = spec_ab(inp)
    a, b = a.double().permute(0, 2, 1, 3), b.double().permute(0, 2, 1, 3)                  # [B, nh, qlen, 64]
    K = inp["K"].double().view(B, klen, nh, 64).permute(0, 2, 1, 3)
    V = inp["V"].double().view(B, klen, nh, 64).permute(0, 2, 1, 3)
    r = inp["r"].double().view(-1, nh, 64).permute(1, 0, 2)                               # [nh, n_dist, 64]
    dist = (torch.arange(qlen)[:, None] + mlen - torch.arange(klen)[None, :]).clamp(min=0)
    ok = allowed_mask(qlen, mlen, shift)
    ac = torch.matmul(a, K.transpose(-1, -2))
    g = torch.matmul(b, r.transpose(-1, -2)[None])
    bd = g.gather(3, dist[None, None].expand(B, nh, qlen, klen))
    mag = torch.matmul(a.abs(), K.abs().transpose(-1, -2)) + torch.matmul(b.abs(), r.abs().transpose(-1, -2)[None]).gather(
        3, dist[None, None].expand(B, nh, qlen, klen))
    sc = ((ac + bd) * scale).masked_fill(~ok, -float("inf"))
    P = torch.softmax(sc, dim=-1)
    return dict(ctx=torch.matmul(P, V), P=P, sc=sc, ok=ok, V=V, mag=mag * abs(scale), mx=sc.amax(-1))


def attn_bar(r, dtype):
    """Per-element bar of ctx; the derivation is in tests/test_gpu_txl_kernels.py."""
    klen = r["sc"].shape[-1]
    half, sub = 2.0 ** -(MANT[dtype] + 1), 2.0 ** (EMIN[dtype] - MANT[dtype] - 1)
    ntile = (klen + TILE - 1) // TILE
    per_wave = (ntile + 3) // 4 + 1
    sc = torch.where(r["ok"], r["sc"], torch.zeros((), dtype=F64))
    A = sc.abs().amax(-1, keepdim=True)
    e_s = 11.0 * U32 * r["mag"]
    e_p = (3.0 * (sc.abs() + r["mx"].abs()[..., None]) + 20.0) * U32 + per_wave * (6.0 * A + 20.0) * U32 + e_s
    P, V = r["P"], r["V"].abs()
    e_l = (P * e_p).sum(-1, keepdim=True) + (18.0 * per_wave + 8.0) * U32
    E = torch.where(r["ok"], e_p + e_l, torch.zeros((), dtype=F64))
    op = torch.where(P == 0, torch.zeros_like(P), torch.clamp_min(half * P, sub))
    n = 3 * ntile + 16
    ref = r["ctx"]
    _, ex = torch.frexp(ref.to(dtype).double().abs())
    ex = torch.where(ref.to(dtype) == 0, torch.full_like(ex, EMIN[dtype] + 1), ex)
    ulp = torch.pow(2.0, (ex - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype])
    return torch.matmul(op, V) + n * U32 * torch.matmul(P, V) + torch.matmul(P * E, V) + ulp + 2 * U32 * ref.abs()


def attn_kernel_model(inp, shift, scale, cap, start, fault=None):
    """The kernel's arithmetic in fp32 on the CPU: per tile of 32 queries the band's key tiles of 32 are dealt round-robin to four
    partial results with their own online maximum, sum and context; probabilities are rounded to the 16-bit type relative to the
    partial's running maximum; the four partials are merged in fixed order; the output is rounded once.  `fault` plants one of
    ATTN_FAULTS.  -> ctx [B, nh, qlen, 64] in `dtype`."""
    B, nh, qlen, mlen, klen, dt = inp["B"], inp["nh"], inp["qlen"], inp["mlen"], inp["klen"], inp["dtype"]
    f32 = torch.float32
    a, b = spec_ab(inp)
    a, b = a.float().permute(0, 2, 1, 3), b.float().permute(0, 2, 1, 3)
    kv = ring_of(inp["K"], inp["V"], cap, start, 0.0)
    H = inp["H"]
    st = (start + 1) % cap if fault == "ring_start" else start
    phys = (st + torch.arange(klen)) % cap
    K = kv[:, phys, :H].float().view(B, klen, nh, 64).permute(0, 2, 1, 3)
    V = kv[:, phys, H:].float().view(B, klen, nh, 64).permute(0, 2, 1, 3)
    r = inp["r"].float().view(-1, nh, 64).permute(1, 0, 2)
    out = torch.zeros(B, nh, qlen, 64, dtype=f32)
    ninf = torch.tensor(-float("inf"), dtype=f32)
    scale32 = torch.tensor(scale, dtype=f32)
    for i0 in range(0, qlen, TILE):
        i1 = min(i0 + TILE, qlen)
        ii = torch.arange(i0, i1)
        jlo, jhi = max(0, i0 - shift + 1), min(klen - 1, i1 - 1 + mlen)
        t0, t1 = jlo // TILE, jhi // TILE
        parts = []
        for w in range(4):
            m = torch.full((B, nh, i1 - i0), -float("inf"), dtype=f32)
            l = torch.zeros(B, nh, i1 - i0, dtype=f32)
            o = torch.zeros(B, nh, i1 - i0, 64, dtype=f32)
            for t in range(t0 + w, t1 + 1, 4):
                jj = torch.arange(t * TILE, min(t * TILE + TILE, klen))
                d = ii[:, None] + mlen - jj[None, :] + (1 if fault == "skew_off_by_one" else 0)
                ac = torch.matmul(a[:, :, i0:i1], K[:, :, jj].transpose(-1, -2))
                g = torch.matmul(b[:, :, i0:i1], r[:, :klen + 2].transpose(-1, -2)[None])
                bd = g.gather(3, d.clamp(min=0, max=klen + 1)[None, None].expand(B, nh, -1, -1))
                x = (ac + bd) * scale32
                up = jj[None, :] <= ii[:, None] + mlen + (1 if fault == "upper_edge" else 0)
                lo = ii[:, None] - shift < jj[None, :] + (1 if fault == "lower_edge" else 0)
                x = torch.where((up & lo)[None, None], x, ninf)
                v = x.amax(-1)
                m_new = torch.maximum(m, v)
                m_use = torch.where(torch.isinf(m_new), torch.zeros((), dtype=f32), m_new)
                alpha = torch.exp((m if fault != "stale_max" else m_new) - m_use)
                p = torch.exp(x - m_use[..., None])
                l = l * alpha + p.sum(-1)
                m = m_new
                p16 = p.to(dt).float()
                o = o * alpha[..., None] + torch.matmul(p16, V[:, :, jj])
            parts.append((m, l, o))
        mt = torch.stack([p[0] for p in parts]).amax(0)
        fs = [torch.where(torch.isinf(m), torch.zeros((), dtype=f32), torch.exp(m - mt)) for m, _, _ in parts]
        lt = sum(l * f for (m, l, o), f in zip(parts, fs))
        acc = torch.zeros(B, nh, i1 - i0, 64, dtype=f32)
        for (m, l, o), f in zip(parts, fs):
            acc = acc + o * (f / lt)[..., None]
        out[:, :, i0:i1] = acc
    return out.to(dt)
