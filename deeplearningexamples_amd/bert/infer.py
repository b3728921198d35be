"""BERT inference on MI355X: encoder features and the pre-training heads, forward only, on PACKED variable-length batches.

Replaces, under model.eval() (LanguageModeling/BERT/):
    modeling.py:285-301,340-434   embeddings and the encoder layers (no dropout)
    modeling.py:518-524,545-595   pooler, MLM head on chosen rows, NSP head
    extract_features.py:262-294   the batch loop: model(input_ids, token_type_ids, attention_mask), the chosen layers per token
The reference pads every sentence to --max_seq_length and runs the [B, S] rectangle through every layer.  Every kernel of the
path but attention is row-wise, so here the encoder runs on the T = sum(len_b) real rows: ids gathered, dle_embed_sum_packed, L
layers on [T, ...] with dle_attention_fwd_varlen (csrc/attention.hip), the pooler on each sequence's first row, and one row
scatter per requested layer back into the padded [B, S, H] form.  The padded path -- the same layer code on B * S rows with
dle_attention_fwd(p = 0, mask_add) inside its envelope and the batched-GEMM pair outside -- stays for masks that are not
prefix-form, for full batches, and as the baseline the packed path is measured against (tools/bert_infer_perf.py).  One host
synchronisation per batch: lengths, prefix-form test and the check of pretraining_logits' positions ride on one transfer.

16-bit GEMM weights only: no fp32 masters of them, no gradients, no saved activations.  HIP-graph replay is out of scope: T
changes per batch.
"""
import math

import torch

from .. import _cabi as C
from .. import functional as F
from .model import BertForPreTraining

# Routing: see DESIGN.md section 4c-2 (measured by tools/bert_infer_perf.py, profiles/bert_infer_perf.json).
PACKED_MAX_FILL = 1.0


# ---------------------------------------------------------------------------------------------------- host-side layout (no kernels)
def inspect_batch(attention_mask, positions=None):
    """-> (lengths: list of B ints, prefix: bool, positions_ok: bool).  prefix: every row of the mask is `len` ones followed by
    zeros.  positions_ok: every flat position (indexes into [B * S]; None: no positions) is in range and at a one of the mask.
    ONE host synchronisation when the mask lives on the device (the cost BertTrainer._prepare_batch pays for its nonzero)."""
    m = attention_mask != 0
    s = m.shape[1]
    lens = m.sum(1)
    want = torch.arange(s, device=m.device)[None, :] < lens[:, None]
    flags = [(m == want).all()]
    if positions is not None and positions.numel():
        pos, n = positions.reshape(-1).to(m.device), m.numel()
        flags.append(((pos >= 0) & (pos < n)).all() & m.reshape(-1)[pos.clamp(0, max(n - 1, 0))].all())
    flat = torch.cat([lens] + [f.to(lens.dtype).reshape(1) for f in flags]).tolist()
    b = lens.numel()
    return [int(x) for x in flat[:b]], bool(flat[b]), all(bool(x) for x in flat[b + 1:])


def lengths_and_prefix(attention_mask):
    """-> (lengths, prefix) of inspect_batch."""
    return inspect_batch(attention_mask)[:2]


def cu_seqlens(lengths, device=None):
    """int32 [B + 1] row offsets of the packed layout: 0, len_0, len_0 + len_1, ..."""
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return torch.tensor(cu, dtype=torch.int32, device=device)


def packed_possible(lengths, prefix, seq_len, varlen_supported):
    """The packed path can run: prefix-form mask, every sequence non-empty, the kernel covers (seq_len, head_dim)."""
    return bool(prefix and varlen_supported and len(lengths) > 0 and min(lengths) >= 1 and max(lengths) <= seq_len)


def padded_supported(seq_len, head_dim, fused_supported):
    """The padded path can run: inside the fused attention kernels, or a key dimension the softmax kernel takes (<= 512)."""
    return bool(fused_supported or (1 << max(seq_len - 1, 1).bit_length()) <= 512)


def choose_packed(lengths, prefix, seq_len, varlen_supported, packed=None, max_fill=PACKED_MAX_FILL, padded_ok=True):
    """The routing rule.  packed=None: packed when possible and T < B * S (fill at most max_fill), or when possible and the
    padded path cannot run at this seq_len (padded_ok False: a full batch at, say, S = 600); True: packed or ValueError; False:
    padded."""
    ok = packed_possible(lengths, prefix, seq_len, varlen_supported)
    if packed is True:
        if not ok:
            raise ValueError("packed=True needs a prefix-form attention mask with no empty sequence and a head size / sequence "
                             "length the packed attention kernel covers")
        return True
    if packed is False or not ok:
        return False
    if not padded_ok:
        return True
    total, full = sum(lengths), len(lengths) * seq_len
    return total < full and total <= max_fill * full


def clean_state_dict(source):
    """A state dict out of a module, a state dict or a {"model": state dict} checkpoint dictionary; a `module.` prefix (DDP) is
    dropped and the tied `cls.predictions.decoder.weight` is left out (it is the word-embedding table)."""
    if isinstance(source, torch.nn.Module):
        source = source.state_dict()
    if isinstance(source, dict) and "model" in source and isinstance(source["model"], dict):
        source = source["model"]
    out = {}
    for k, v in source.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k != "cls.predictions.decoder.weight":
            out[k] = v
    return out


def resolve_layers(layers, n_layers):
    """Reference layer indexes (-1 = last encoder layer, extract_features.py --layers) -> 0 .. n_layers - 1."""
    out = []
    for l in layers:
        if not -n_layers <= l < n_layers:
            raise ValueError("layer index %d outside a %d-layer encoder" % (l, n_layers))
        out.append(l % n_layers)
    return out


class BertPredictor:
    """Forward-only BERT.  `source`: a BertForPreTraining module, a state dict, or a checkpoint dictionary with a "model" key;
    `config`: the model.py configuration dictionary (taken from the module when one is given).  A source without the `cls.*`
    heads loads as encoder-only (encode works, pretraining_logits raises)."""

    def __init__(self, source, config=None, compute_dtype=torch.float16, device="cuda"):
        if isinstance(source, BertForPreTraining) and config is None:
            config = source.config
        if config is None:
            raise ValueError("BertPredictor needs the model configuration when it is not built from a BertForPreTraining module")
        self.cfg, self.dtype, self.dev = dict(config), compute_dtype, torch.device(device)
        sd = clean_state_dict(source)
        h, dev = self.cfg["hidden"], self.dev
        f32 = lambda k: sd[k].detach().to(device=dev, dtype=torch.float32).contiguous()
        w16 = lambda k: F.cast(f32(k), compute_dtype)
        e = "bert.embeddings."
        self.word, self.pos, self.typ = f32(e + "word_embeddings.weight"), f32(e + "position_embeddings.weight"), f32(e + "token_type_embeddings.weight")
        self.ln0 = (f32(e + "LayerNorm.weight"), f32(e + "LayerNorm.bias"))
        self.layers = []
        for l in range(self.cfg["layers"]):
            p = "bert.encoder.layer.%d." % l
            qkv = torch.cat([f32(p + "attention.self.%s.weight" % n) for n in ("query", "key", "value")], 0)
            self.layers.append(dict(
                qkv=F.cast(qkv, compute_dtype), qkv_b=torch.cat([f32(p + "attention.self.%s.bias" % n) for n in ("query", "key", "value")], 0),
                ao=w16(p + "attention.output.dense.weight"), ao_b=f32(p + "attention.output.dense.bias"),
                ln1=(f32(p + "attention.output.LayerNorm.weight"), f32(p + "attention.output.LayerNorm.bias")),
                ff1=w16(p + "intermediate.dense_act.weight"), ff1_b=f32(p + "intermediate.dense_act.bias"),
                ff2=w16(p + "output.dense.weight"), ff2_b=f32(p + "output.dense.bias"),
                ln2=(f32(p + "output.LayerNorm.weight"), f32(p + "output.LayerNorm.bias"))))
            del qkv
        self.pool, self.pool_b = w16("bert.pooler.dense_act.weight"), f32("bert.pooler.dense_act.bias")
        self.has_heads = "cls.predictions.bias" in sd
        if self.has_heads:
            t = "cls.predictions.transform."
            self.tr, self.tr_b = w16(t + "dense_act.weight"), f32(t + "dense_act.bias")
            self.tr_ln = (f32(t + "LayerNorm.weight"), f32(t + "LayerNorm.bias"))
            v = self.word.shape[0]
            self.vocab, vp = v, (v + 7) // 8 * 8
            self.dec = torch.zeros((vp, h), dtype=compute_dtype, device=dev)           # tied decoder, rows padded to 8
            F.cast(self.word, compute_dtype, out=self.dec[:v])
            self.dec_b = torch.zeros(vp, dtype=torch.float32, device=dev)
            self.dec_b[:v].copy_(f32("cls.predictions.bias"))
            self.nsp = torch.zeros((8, h), dtype=compute_dtype, device=dev)            # 2 -> 8 rows, as in the train step
            F.cast(f32("cls.seq_relationship.weight"), compute_dtype, out=self.nsp[:2])
            self.nsp_b = torch.zeros(8, dtype=torch.float32, device=dev)
            self.nsp_b[:2].copy_(f32("cls.seq_relationship.bias"))
        self.last_route = None          # "packed" / "padded": what the last batch took

    # ------------------------------------------------------------------ attention of the two layouts
    def _attention_padded(self, qkv, mask_add, b, s):
        h, nh = self.cfg["hidden"], self.cfg["heads"]
        d = h // nh
        scale = 1.0 / math.sqrt(d)
        if F.attention_supported(s, d):
            return F.attention_fwd(qkv, mask_add, b, s, nh, scale, p=0.0)[0]
        # outside the fused envelope: scores through HBM.  The softmax kernel takes rows of a power-of-two length: the key
        # dimension is padded to it with zero scores under a -10000 mask
        lk = 1 << max(s - 1, 1).bit_length()
        if lk > 512:
            raise ValueError("padded attention: sequence length %d is outside the fused kernels (multiples of 128) and the "
                             "softmax kernel (<= 512)" % s)
        probs = torch.zeros((b * nh, s, lk), dtype=self.dtype, device=self.dev)
        F.gemm_batched(qkv, qkv[:, h:], probs, s, s, d, 3 * h, 3 * h, lk, True, True, b * nh, nh,
                       (s * 3 * h, d), (s * 3 * h, d), (nh * s * lk, s * lk))
        mk = torch.full((b, lk), -10000.0, dtype=torch.float32, device=self.dev)
        mk[:, :s] = mask_add
        F.softmax_fwd_(probs, mk, nh * s, scale)
        ctx = torch.empty((b * s, h), dtype=self.dtype, device=self.dev)
        F.gemm_batched(probs, qkv[:, 2 * h:], ctx, s, d, s, lk, 3 * h, h, True, False, b * nh, nh,
                       (nh * s * lk, s * lk), (s * 3 * h, d), (s * h, d))
        return ctx

    def _packed_rows(self, cu, total, s):
        """int64 flat indexes into [B * S] of the packed rows of a prefix-form mask, built on the device from cu_seqlens (no
        host synchronisation): packed row t of sequence b sits at b * S + t - cu[b]."""
        t = torch.arange(total, device=self.dev, dtype=torch.int64)
        seq = torch.searchsorted(cu[1:].to(torch.int64), t, right=True)
        return t + seq * s - cu.to(torch.int64)[seq]

    def _mask_rows(self, attention_mask, total):
        """The same for any mask (row-major order of its ones) without a second host synchronisation: their number is known, so a
        stable sort on the device stands in for nonzero."""
        order = torch.sort((attention_mask.reshape(-1) == 0).to(torch.int8), stable=True).indices
        return order[:total].contiguous()

    # ------------------------------------------------------------------ the forward pass
    def _forward(self, input_ids, token_type_ids, attention_mask, packed, want, positions=None):
        """-> dict(route, b, s, rows (packed route: flat indexes of the mask's ones, packed order), hidden {layer: [rows of that
        route, H]}, x (last layer), pooled [B, H]).  `want`: resolved layer indexes whose output is kept; `positions`: flat
        indexes that must lie at ones of the mask (checked in the batch's one host synchronisation)."""
        cfg, dt, dev = self.cfg, self.dtype, self.dev
        h, nh, inter = cfg["hidden"], cfg["heads"], cfg["intermediate"]
        d = h // nh
        b, s = input_ids.shape
        if s > self.pos.shape[0]:
            raise ValueError("sequence length %d above the %d position embeddings" % (s, self.pos.shape[0]))
        input_ids, token_type_ids, attention_mask = (x.to(dev) for x in (input_ids, token_type_ids, attention_mask))
        lengths, prefix, positions_ok = inspect_batch(attention_mask, positions)
        if not positions_ok:
            raise ValueError("pretraining_logits: a position lies outside the batch or points at a padding token")
        use_packed = choose_packed(lengths, prefix, s, F.attention_varlen_supported(s, d), packed,
                                   padded_ok=padded_supported(s, d, F.attention_supported(s, d)))
        ids, tts = input_ids.reshape(-1).contiguous(), token_type_ids.reshape(-1).contiguous()
        rows = None
        if use_packed:
            t = sum(lengths)
            cu = cu_seqlens(lengths, dev)
            rows = self._packed_rows(cu, t, s)
            z0 = F.embed_sum_packed(self.word, self.pos, self.typ, ids[rows].contiguous(), tts[rows].contiguous(),
                                    (rows % s).to(torch.int32), dt)
            idx0 = cu[:-1].to(torch.int64)
            max_len, scale = max(lengths), 1.0 / math.sqrt(d)
            attn = lambda qkv: F.attention_fwd_varlen(qkv, cu, max_len, nh, scale)
        else:
            t = b * s
            z0 = F.embed_sum(self.word, self.pos, self.typ, ids, tts, s, dt)
            idx0 = torch.arange(b, device=dev, dtype=torch.int64) * s
            mask_add = ((1.0 - (attention_mask != 0).to(torch.float32)) * -10000.0).contiguous()
            attn = lambda qkv: self._attention_padded(qkv, mask_add, b, s)
        x = F.layernorm_fwd(z0, self.ln0[0], self.ln0[1])[0]
        hidden = {}
        for l, w in enumerate(self.layers):
            qkv = F.gemm(x, w["qkv"], t, 3 * h, h, True, True, bias=w["qkv_b"])
            ctx = attn(qkv)
            ao = F.gemm(ctx, w["ao"], t, h, h, True, True, bias=w["ao_b"])
            x1 = F.layernorm_fwd(ao, w["ln1"][0], w["ln1"][1], residual=x, write_z=False)[0]
            it = F.gemm(x1, w["ff1"], t, inter, h, True, True, bias=w["ff1_b"], act=C.ACT_GELU)
            o2 = F.gemm(it, w["ff2"], t, h, inter, True, True, bias=w["ff2_b"])
            x = F.layernorm_fwd(o2, w["ln2"][0], w["ln2"][1], residual=x1, write_z=False)[0]
            if l in want:
                hidden[l] = x
        first = F.rows_gather(x, idx0)
        pooled = F.gemm(first, self.pool, b, h, h, True, True, bias=self.pool_b, act=C.ACT_TANH)
        self.last_route = "packed" if use_packed else "padded"
        return dict(route=self.last_route, b=b, s=s, rows=rows, hidden=hidden, x=x, pooled=pooled, total=sum(lengths),
                    mask=attention_mask)

    def _to_padded(self, r, x):
        """Rows of the route's layout -> [B, S, H] with zeros at the padding positions."""
        b, s, h = r["b"], r["s"], self.cfg["hidden"]
        if r["route"] == "padded" and r["total"] == b * s:
            return x.view(b, s, h)
        out = torch.zeros((b * s, h), dtype=x.dtype, device=x.device)
        if r["route"] == "packed":
            F.rows_scatter_(out, x, r["rows"])
        elif r["total"]:
            if r["rows"] is None:                       # a padded batch with padding: the row list is built once, here
                r["rows"] = self._mask_rows(r["mask"], r["total"])
            F.rows_scatter_(out, F.rows_gather(x, r["rows"]), r["rows"])
        return out.view(b, s, h)

    def encode(self, input_ids, token_type_ids, attention_mask, layers=(-1,), packed=None):
        """-> ([hidden states [B, S, H] of the chosen encoder layers, zeros at padding], pooled output [B, H])."""
        want = resolve_layers(layers, self.cfg["layers"])
        r = self._forward(input_ids, token_type_ids, attention_mask, packed, set(want))
        return [self._to_padded(r, r["hidden"][l]) for l in want], r["pooled"]

    def pretraining_logits(self, input_ids, token_type_ids, attention_mask, positions, packed=None):
        """-> (fp32 MLM logits [n, vocab] at the flat positions (indexes into [B * S], all at unmasked tokens), fp32 NSP logits
        [B, 2])."""
        if not self.has_heads:
            raise ValueError("this checkpoint has no cls.* heads: encoder-only")
        sel = positions.to(self.dev).reshape(-1).to(torch.int64)
        r = self._forward(input_ids, token_type_ids, attention_mask, packed, set(), positions=sel)
        h = self.cfg["hidden"]
        if r["route"] == "packed":                      # flat [B * S] index -> packed row (the positions were checked above)
            inv = torch.zeros((r["b"] * r["s"],), dtype=torch.int64, device=self.dev)
            inv[r["rows"]] = torch.arange(r["rows"].numel(), device=self.dev, dtype=torch.int64)
            sel = inv[sel]
        n = sel.numel()
        hm = F.rows_gather(r["x"], sel.contiguous())
        tg = F.gemm(hm, self.tr, n, h, h, True, True, bias=self.tr_b, act=C.ACT_GELU)
        tl = F.layernorm_fwd(tg, self.tr_ln[0], self.tr_ln[1])[0]
        logits = F.gemm(tl, self.dec, n, self.dec.shape[0], h, True, True, out_dtype=torch.float32, bias=self.dec_b)
        nsp = F.gemm(r["pooled"], self.nsp, r["b"], 8, h, True, True, out_dtype=torch.float32, bias=self.nsp_b)
        return logits[:, :self.vocab], nsp[:, :2]
