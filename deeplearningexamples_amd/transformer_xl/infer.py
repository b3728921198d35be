"""Transformer-XL evaluation with memory on the gfx950 library: MemTransformerLM.forward of
LanguageModeling/Transformer-XL/pytorch/mem_transformer.py:684-800 (attn_type 0, post-LayerNorm, evaluation mode) with the loss of
utils/proj_adaptive_softmax.py:131-208, one segment at a time.

What is cached.  The reference keeps the HIDDEN states of the last mem_len positions per layer and projects all mlen + qlen of them
to K and V again in every segment (`qkv_net(cat([mems, w]))`, :239-247).  Memory rows are inputs of a frozen row-wise linear map, so
this keeps their K and V instead: per layer a ring [bsz, cap = mem_len + tgt_len, 2H] plus two host integers, `start` and `mlen`.
A segment appends its qlen rows behind the window and then drops what no longer fits (`_update_mems`, :652-682 for ext_len 0:
mlen' = min(mem_len, mlen + qlen); start advances by what fell out).  `r_net(pos_emb)` depends on the distance only: the table of
every layer is computed once at construction for all mem_len + tgt_len distances (the reference rebuilds it per segment, :707-711, :244).

Layout.  Activations are 16-bit [bsz * qlen, d_model], rows BATCH-major (row = b * qlen + t), so that a (batch element, head) pair
of the attention kernel walks contiguous query rows; the loss comes back in the reference's [qlen, bsz] order.

Launches of a segment, for L layers, C tail clusters that have rows, div_val 1 with d_embed == d_model (the WikiText-103 models):
  1        dle_rows_gather_scale        embedding rows times sqrt(d_model)
  L x      dle_gemm                     QKV of the NEW rows only
           dle_txl_kv_append            their K | V thirds -> the ring
           dle_txl_rel_attention_fwd    AC + shifted BD, mask, softmax, context in one launch
           dle_gemm                     o_net
           dle_layernorm_fwd            LayerNorm(x + attn_out)
           dle_gemm, dle_gemm           the feed-forward, ReLU in the first epilogue
           dle_layernorm_fwd            LayerNorm(x + ff)
  1        dle_gemm                     head logits (shortlist + clusters), fp32, all rows
  1        dle_row_nll                  the head part of every token's loss
  C x      dle_rows_gather_scale, dle_gemm, dle_row_nll (accumulate)      the rows of one cluster: gather, tail logits, tail part
With div_val > 1 (or d_embed != d_model) each bucket of the embedding and of the softmax has one more dle_gemm, its projection.

Host synchronisation.  The iterator hands data and target over on the HOST, so both adaptive layers are bucketed there, before the
ids are uploaded: every index list of a segment travels in ONE host-to-device copy and nothing is read back.  The loss stays on
the device; the caller reads it when it wants to (`eval.py`: once per --log_interval).

Not built (one-line errors): fp32, what model.check_config rejects, segments longer than tgt_len.  No CPU path.
"""
import math

import numpy as np
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import gpu_device, require_16bit
from .model import TransformerXLModel

LN_EPS = 1e-5          # nn.LayerNorm's default, which the reference uses


class _Layer:
    __slots__ = ("qkv", "o", "ln1", "ff1", "ff2", "ln2", "r", "kv")


class TransformerXLEvaluator:
    def __init__(self, model, batch_size, tgt_len=None, mem_len=None, dtype=torch.float16, device=None):
        """model: a TransformerXLModel (left untouched).  tgt_len / mem_len default to the configuration's."""
        require_16bit(dtype, "TransformerXLEvaluator")
        if not isinstance(model, TransformerXLModel):
            raise TypeError("model must be a TransformerXLModel")
        cfg = self.cfg = model.cfg
        self.tgt_len = int(cfg["tgt_len"] if tgt_len is None else tgt_len)
        self.mem_len = int(cfg["mem_len"] if mem_len is None else mem_len)
        self.bsz = int(batch_size)
        if self.bsz < 1 or self.tgt_len < 1 or self.mem_len < 0:
            raise ValueError("batch_size and tgt_len must be positive, mem_len not negative")
        self.cap = self.mem_len + self.tgt_len
        if not F.txl_attention_supported(self.tgt_len, self.cap, cfg["d_head"]):
            raise ValueError("tgt_len %d with mem_len %d is outside the attention kernel's envelope (tgt_len <= 512, "
                             "mem_len + tgt_len <= 4096)" % (self.tgt_len, self.mem_len))
        self.dev = dev = gpu_device(device, "TransformerXLEvaluator")
        self.dtype = dtype
        self.nh, self.H, self.d_model = cfg["n_head"], cfg["n_head"] * cfg["d_head"], cfg["d_model"]
        self.scale = 1.0 / math.sqrt(cfg["d_head"])
        self.emb_scale = float(cfg["d_model"]) ** 0.5
        self.ends, self.ncl = model.ends, model.n_clusters
        self.head_size = self.ends[1] + self.ncl - 1
        P = model.params
        w16 = lambda t: t.to(dtype).contiguous().to(dev)
        f32 = lambda t: t.to(torch.float32).contiguous().to(dev)
        with torch.no_grad():
            # adaptive embedding: tables and projections as the reference holds them
            self.div1 = cfg["div_val"] == 1
            n_emb = 1 if self.div1 else self.ncl
            self.emb = [w16(P["word_emb.emb_layers.%d.weight" % i]) for i in range(n_emb)]
            self.emb_proj = [w16(P["word_emb.emb_projs.%d" % i]) if ("word_emb.emb_projs.%d" % i) in P else None for i in range(n_emb)]
            # adaptive softmax: head = cat(W[:c0], cluster_weight); tails; the projections transposed once ([d_emb_i, d_model])
            self.out_w, self.out_b, self.out_proj = [], [], []
            for i in range(self.ncl):
                w, b = model.out_weight(i)
                if i == 0 and self.ncl > 1:
                    w = torch.cat([w, P["crit.cluster_weight"]], 0)
                    b = torch.cat([b, P["crit.cluster_bias"]], 0)
                pr = model.out_proj(i)
                self.out_w.append(w16(w))
                self.out_b.append(f32(b))
                self.out_proj.append(None if pr is None else w16(pr.t()))
            self.u, self.v = w16(P["r_w_bias"]), w16(P["r_r_bias"])
            # the distance tables: r[d] = r_net(pos_emb(min(d, clamp_len))), d < mem_len + tgt_len, once
            d = torch.arange(self.cap, dtype=torch.float64)
            if cfg["clamp_len"] > 0:
                d = d.clamp(max=cfg["clamp_len"])
            sin_inp = torch.outer(d, P["pos_emb.inv_freq"].double())
            pos = w16(torch.cat([sin_inp.sin(), sin_inp.cos()], dim=-1))
            self.layers = []
            for l in range(cfg["n_layer"]):
                p, L = "layers.%d." % l, _Layer()
                L.qkv, L.o = w16(P[p + "dec_attn.qkv_net.weight"]), w16(P[p + "dec_attn.o_net.weight"])
                L.ln1 = (f32(P[p + "dec_attn.layer_norm.weight"]), f32(P[p + "dec_attn.layer_norm.bias"]))
                L.ff1 = (w16(P[p + "pos_ff.CoreNet.0.weight"]), f32(P[p + "pos_ff.CoreNet.0.bias"]))
                L.ff2 = (w16(P[p + "pos_ff.CoreNet.3.weight"]), f32(P[p + "pos_ff.CoreNet.3.bias"]))
                L.ln2 = (f32(P[p + "pos_ff.layer_norm.weight"]), f32(P[p + "pos_ff.layer_norm.bias"]))
                rn = w16(P[p + "dec_attn.r_net.weight"])
                L.r = F.gemm(pos, rn, self.cap, self.H, self.d_model, True, True)
                L.kv = torch.zeros((self.bsz, self.cap, 2 * self.H), dtype=dtype, device=dev)
                self.layers.append(L)
        self.start, self.mlen = 0, 0

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, batch_size, tgt_len, mem_len, clamp_len=-1, same_length=False, **kw):
        """eval.py:385-394: the checkpoint's model_config with the evaluation lengths of the command line."""
        model, vocab, args = TransformerXLModel.from_checkpoint(path_or_ckpt, tgt_len=tgt_len, ext_len=0, mem_len=mem_len,
                                                                clamp_len=clamp_len, same_length=same_length)
        ev = cls(model, batch_size, **kw)
        ev.vocab, ev.args = vocab, args
        return ev

    def reset(self):
        """Forget the memory (the rings are zero-filled again, as at construction)."""
        for L in self.layers:
            L.kv.zero_()
        self.start, self.mlen = 0, 0

    # ------------------------------------------------------------------ host bucketing
    def bucket(self, data, target):
        """Every index list of a segment, from the HOST ids [qlen, bsz]: -> (one int32 array, a plan of offsets into it).
        Rows are batch-major (row = b * qlen + t); loss positions follow the reference's [qlen, bsz] order (t * bsz + b)."""
        qlen, bsz = data.shape
        tok = np.ascontiguousarray(data.t().numpy()).reshape(-1)
        tgt = np.ascontiguousarray(target.t().numpy()).reshape(-1)
        n_token = self.ends[-1]
        if tok.min() < 0 or tok.max() >= n_token or tgt.min() < 0 or tgt.max() >= n_token:
            raise ValueError("token ids must be in [0, %d)" % n_token)
        rows = np.arange(qlen * bsz, dtype=np.int64)
        pos = (rows % qlen) * bsz + rows // qlen
        parts, plan, off = [], {"emb": [], "tails": []}, 0

        def put(a):
            nonlocal off
            a = np.asarray(a, dtype=np.int32)
            parts.append(a)
            off += a.size
            return (off - a.size, a.size)

        if self.div1:
            plan["emb"].append((0, put(tok), None))
        else:
            which = np.searchsorted(np.asarray(self.ends[1:]), tok, side="right")
            for i in range(self.ncl):
                r = rows[which == i]
                if r.size:
                    plan["emb"].append((i, put(tok[r] - self.ends[i]), put(r)))
        cl = np.searchsorted(np.asarray(self.ends[1:]), tgt, side="right")
        plan["head"] = (put(np.where(cl == 0, tgt, self.head_size - cl)), put(pos))
        for i in range(1, self.ncl):
            r = rows[cl == i]
            if r.size:
                plan["tails"].append((i, put(r), put(tgt[r] - self.ends[i]), put(pos[r])))
        return np.concatenate(parts), plan

    # ------------------------------------------------------------------ one segment
    def segment(self, data, target):
        """data, target: HOST int64 [qlen, bsz] (qlen <= tgt_len; what LMOrderedIterator yields) -> nll fp32 [qlen, bsz] on the
        device; the memory moves on by qlen positions."""
        if data.is_cuda or target.is_cuda:
            raise ValueError("segment takes the ids on the host (the adaptive layers are bucketed there)")
        if data.dim() != 2 or tuple(data.shape) != tuple(target.shape) or data.dtype != torch.int64 or target.dtype != torch.int64:
            raise ValueError("data and target must be int64 [qlen, bsz] of one shape")
        qlen, bsz = data.shape
        if bsz != self.bsz or not (1 <= qlen <= self.tgt_len):
            raise ValueError("segment of [%d, %d]: the evaluator was built for batch %d and at most %d positions"
                             % (qlen, bsz, self.bsz, self.tgt_len))
        dev, dt, R, dm = self.dev, self.dtype, qlen * bsz, self.d_model
        host, plan = self.bucket(data, target)
        mlen, start = self.mlen, self.start
        klen = mlen + qlen
        if self.cfg["same_length"]:                                   # mem_transformer.py:691-699
            mask_len = klen - self.mem_len - 1
            shift = qlen - mask_len if mask_len > 0 else qlen
        else:
            shift = qlen
        with torch.no_grad():
            idx = torch.from_numpy(host).to(dev, non_blocking=True)                  # the segment's one upload
            cut = lambda s: idx[s[0]:s[0] + s[1]]
            # ---- adaptive embedding
            x = torch.empty((R, dm), dtype=dt, device=dev)
            for i, src, dst in plan["emb"]:
                n = src[1]
                proj = self.emb_proj[i]
                if proj is None:
                    F.rows_gather_scale(self.emb[i], x, n, src_idx=cut(src), dst_idx=None if dst is None else cut(dst),
                                        scale=self.emb_scale)
                else:
                    e = torch.empty((n, self.emb[i].shape[1]), dtype=dt, device=dev)
                    F.rows_gather_scale(self.emb[i], e, n, src_idx=cut(src))
                    pe = F.gemm(e, proj, n, dm, e.shape[1], True, True)
                    F.rows_gather_scale(pe, x, n, dst_idx=None if dst is None else cut(dst), scale=self.emb_scale)
            # ---- the layers
            for L in self.layers:
                qkv = F.gemm(x, L.qkv, R, 3 * self.H, dm, True, True)
                F.txl_kv_append(qkv, L.kv, qlen, mlen, start)
                ctx = F.txl_rel_attention_fwd(qkv[:, :self.H], self.u, self.v, L.kv, L.r, self.nh, qlen, mlen, start, shift,
                                              self.scale)
                ao = F.gemm(ctx, L.o, R, dm, self.H, True, True)
                x = F.layernorm_fwd(ao, L.ln1[0], L.ln1[1], residual=x, eps=LN_EPS, write_z=False)[0]
                h1 = F.gemm(x, L.ff1[0], R, L.ff1[0].shape[0], dm, True, True, bias=L.ff1[1], act=C.ACT_RELU)
                h2 = F.gemm(h1, L.ff2[0], R, dm, h1.shape[1], True, True, bias=L.ff2[1])
                x = F.layernorm_fwd(h2, L.ln2[0], L.ln2[1], residual=x, eps=LN_EPS, write_z=False)[0]
            # ---- adaptive softmax, keep_order
            nll = torch.empty(R, dtype=torch.float32, device=dev)
            F.row_nll(self._logits(x, 0, R), cut(plan["head"][0]), nll, pos=cut(plan["head"][1]))
            for i, rows, tgt, pos in plan["tails"]:
                n = rows[1]
                hi = torch.empty((n, dm), dtype=dt, device=dev)
                F.rows_gather_scale(x, hi, n, src_idx=cut(rows))
                F.row_nll(self._logits(hi, i, n), cut(tgt), nll, pos=cut(pos), accumulate=True)
        # ---- _update_mems for ext_len == 0: the window keeps its last mem_len positions
        self.mlen = min(self.mem_len, klen)
        self.start = (start + klen - self.mlen) % self.cap
        return nll.view(qlen, bsz)

    def _logits(self, hidden, i, n):
        """fp32 logits of cluster i (0: the head) for n rows (proj_adaptive_softmax.py:111-118)."""
        if self.out_proj[i] is not None:
            pt = self.out_proj[i]
            hidden = F.gemm(hidden, pt, n, pt.shape[0], pt.shape[1], True, True)
        w = self.out_w[i]
        return F.gemm(hidden, w, n, w.shape[0], w.shape[1], True, True, out_dtype=torch.float32, bias=self.out_b[i])
