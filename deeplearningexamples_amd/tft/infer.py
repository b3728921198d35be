"""Temporal Fusion Transformer forecasts on the gfx950 library: TemporalFusionTransformer.forward of
PyTorch/Forecasting/TFT/modeling.py:454-468 (with TFTBack.forward :393-432) in evaluation mode, hidden size 128.

Launches of one forecast (17; the reference runs several hundred):
  1   static selection      dle_tft_grn_fwd with a row index list (one static categorical: the selection weight is exactly 1 and the
                            network is the variable's GRN on the gathered embedding rows), or dle_tft_vsn_fwd (static continuous)
  4   dle_tft_grn_fwd       the context networks cs, ce, ch, cc on [B, 128]
  2   dle_tft_vsn_fwd       history (observed | known | target columns, steps < encoder_length) and future (known, the rest):
                            embedding, joint network, softmax, the variables' networks and the weighted sum; both write into one
                            [B, T, 128] tensor
  1   dle_gemm              the input projections of BOTH encoders for all B T rows, fp32 [B T, 1024] (W_ih of the history encoder
                            stacked on the future encoder's; each LSTM reads its half at its steps: one launch instead of two,
                            for 2 x the products of a GEMM that takes microseconds)
  2   dle_tft_lstm_fwd      history, then future from the history's last h (16 bits) and c (fp32); both write into one [B, T, 128]
  1   dle_tft_grn_fwd       input gate + skip connection + LayerNorm (gate mode)
  1   dle_tft_grn_fwd       static enrichment with ce
  1   dle_gemm              q | k | v of all rows
  1   dle_tft_attention_fwd the decoder positions only
  3   dle_tft_grn_fwd       attention gate, position-wise network, decoder gate with the quantile projection as its tail
From the attention on every launch works on B (T - encoder_length) rows.  Nothing is read back: the forecasts stay on the device.
explain=True adds no launch: the selection and attention kernels write the weights they compute anyway.

Not built (one-line errors): hidden sizes other than 128, head counts other than 4, temporal categorical inputs, static inputs
that mix categorical and continuous variables or hold several categoricals, more than 8 variables per selection network,
example lengths above 192, fp32.  No CPU path.
"""
import torch

from .. import functional as F
from ..utils.frontend import GraphCache, gpu_device, require_16bit
from .model import LN_EPS, TemporalFusionTransformer


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


class TFTForecaster:
    def __init__(self, model, dtype=torch.float16, device=None, graphs=False):
        """model: a TemporalFusionTransformer (left untouched).  Weights are packed once, here.  graphs: replay one captured graph
        per (batch size, T, explain); the chain is one stream, no branches."""
        require_16bit(dtype, "TFTForecaster")
        if not isinstance(model, TemporalFusionTransformer):
            raise TypeError("model must be a TemporalFusionTransformer")
        self.dev = dev = gpu_device(device, "TFTForecaster")
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        back = model.TFTpart2
        H = back.quantile_proj.in_features
        if H != F.TFT_HIDDEN:
            raise ValueError("TFTForecaster: the kernels are built for hidden_size 128 (got %d)" % H)
        if back.attention.n_head != 4:
            raise ValueError("TFTForecaster: the attention kernel is built for 4 heads (got %d)" % back.attention.n_head)
        self.dtype, self.enc = dtype, int(model.encoder_length)
        self._graphs = GraphCache(graphs)     # (B, T, explain) -> GraphedStep
        emb = model.embedding
        n_cat = len(emb.s_cat_embed) if emb.s_cat_embed is not None else 0
        n_scont = emb.s_cont_embedding_vectors.shape[0] if emb.s_cont_embedding_vectors is not None else 0
        if not ((n_cat == 1 and n_scont == 0) or (n_cat == 0 and n_scont >= 1)):
            raise ValueError("TFTForecaster: static inputs must be one categorical variable or continuous variables only "
                             "(got %d categorical, %d continuous)" % (n_cat, n_scont))
        with torch.no_grad():
            grn = lambda prefix: F.tft_grn_pack(_sub(sd, prefix), dtype, dev)
            gate = lambda glu, ln: F.tft_grn_pack({"glu.lin.weight": sd[glu + ".lin.weight"], "glu.lin.bias": sd[glu + ".lin.bias"],
                                                   "layer_norm.ln.weight": sd[ln + ".weight"], "layer_norm.ln.bias": sd[ln + ".bias"]}, dtype, dev)
            e, P = "embedding.", "TFTpart2."
            if n_cat:
                self.s_table = sd[e + "s_cat_embed.0.weight"].to(device=dev, dtype=dtype).contiguous()
                self.s_grn = grn("static_encoder.vsn.var_grns.0.")
                self.s_vsn = None
            else:
                svsn = {k: v for k, v in _sub(sd, "static_encoder.vsn.").items() if k != "joint_grn.lin_c.weight"}   # never used: no context
                self.s_vsn = F.tft_vsn_pack(svsn, sd[e + "s_cont_embedding_vectors"], sd[e + "s_cont_embedding_bias"], dtype, dev)
            self.ctx_grns = [grn("static_encoder.context_grns.%d." % i) for i in range(4)]
            # history columns in the reference's order: observed, known, target (modeling.py:462-466)
            self.has_obs = emb.t_cont_o_embedding_vectors is not None
            if emb.t_cont_k_embedding_vectors is None:
                raise ValueError("TFTForecaster: the model has no known continuous input, so no future input")
            names = (["t_cont_o"] if self.has_obs else []) + ["t_cont_k", "t_tgt"]
            vec = torch.cat([sd[e + n + "_embedding_vectors"] for n in names])
            bias = torch.cat([sd[e + n + "_embedding_bias"] for n in names])
            self.hist_vsn = F.tft_vsn_pack(_sub(sd, P + "history_vsn."), vec, bias, dtype, dev)
            self.fut_vsn = F.tft_vsn_pack(_sub(sd, P + "future_vsn."), sd[e + "t_cont_k_embedding_vectors"], sd[e + "t_cont_k_embedding_bias"],
                                          dtype, dev)
            w = lambda k: sd[k].to(device=dev, dtype=dtype).contiguous()
            f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
            self.w_ih = torch.cat([w(P + "history_encoder.weight_ih_l0"), w(P + "future_encoder.weight_ih_l0")]).contiguous()
            self.b_ih = f32(torch.cat([sd[P + "history_encoder.bias_ih_l0"] + sd[P + "history_encoder.bias_hh_l0"],
                                       sd[P + "future_encoder.bias_ih_l0"] + sd[P + "future_encoder.bias_hh_l0"]]))
            self.w_hh = [w(P + "history_encoder.weight_hh_l0"), w(P + "future_encoder.weight_hh_l0")]
            self.input_gate = gate(P + "input_gate", P + "input_gate_ln")
            self.enrichment = grn(P + "enrichment_grn.")
            self.w_qkv, self.w_o = w(P + "attention.qkv_linears.weight"), w(P + "attention.out_proj.weight")
            self.attention_gate = gate(P + "attention_gate", P + "attention_ln")
            self.positionwise = grn(P + "positionwise_grn.")
            self.decoder_gate = gate(P + "decoder_gate", P + "decoder_ln")
            self.wq, self.bq = f32(sd[P + "quantile_proj.weight"]), f32(sd[P + "quantile_proj.bias"])

    def _f32(self, t):
        return None if t is None else t.to(device=self.dev, dtype=torch.float32).contiguous()

    def forecast(self, batch, explain=False):
        """batch: the reference's dictionary (s_cat, s_cont, k_cont, o_cont, target; absent entries None), tensors [B, T, n].
        -> forecasts [B, T - encoder_length, Q] fp32 on the device; with explain=True also the history and future selection
        weights ([B, encoder_length, F_hist], [B, T - encoder_length, F_fut]) and the mean attention probabilities
        [B, T - encoder_length, T], all fp32.  With graphs=True the tensors are the graph's static outputs: copy them before the
        next call of the same shape."""
        if batch.get("k_cat") is not None or batch.get("o_cat") is not None:
            raise NotImplementedError("TFTForecaster: temporal categorical inputs (k_cat / o_cat) are not supported")
        target, known, observed = self._f32(batch["target"]), self._f32(batch.get("k_cont")), self._f32(batch.get("o_cont"))
        B, T = target.shape[0], target.shape[1]
        if not self.enc < T <= 192:
            raise ValueError("TFTForecaster: needs encoder_length %d < T <= 192 (got T %d)" % (self.enc, T))
        if (observed is not None) != self.has_obs or known is None:
            raise ValueError("TFTForecaster: the batch's continuous inputs do not match the model's")
        if self.s_vsn is None:
            static = batch["s_cat"][:, 0, 0].to(device=self.dev, dtype=torch.int32).contiguous()
        else:
            static = self._f32(batch["s_cont"])
        return self._graphs.run((B, T, bool(explain)), lambda s, k, o, t: self._run(s, k, o, t, explain),
                                static, known, observed, target)

    def _run(self, static, known, observed, target, explain):
        H, enc, dt = F.TFT_HIDDEN, self.enc, self.dtype
        B, T = target.shape[0], target.shape[1]
        nq = T - enc
        # static path
        if self.s_vsn is None:
            sctx = F.tft_grn_fwd(self.s_table, self.s_grn, x_index=static, eps=LN_EPS)
        else:
            sctx = F.tft_vsn_fwd([static], self.s_vsn, dt, 1, eps=LN_EPS).view(B, H)
        cs, ce, ch, cc = (F.tft_grn_fwd(sctx, p, eps=LN_EPS) for p in self.ctx_grns)
        # variable selection, both windows into one tensor
        feat = torch.empty((B, T, H), dtype=dt, device=self.dev)
        r = F.tft_vsn_fwd([observed, known, target], self.hist_vsn, dt, enc, ctx=cs, out=feat, want_weights=explain, eps=LN_EPS)
        hist_w = r[1] if explain else None
        r = F.tft_vsn_fwd([known], self.fut_vsn, dt, nq, t0=enc, ctx=cs, out=feat, out_t0=enc, want_weights=explain, eps=LN_EPS)
        fut_w = r[1] if explain else None
        # the two encoders
        xp = F.gemm(feat.view(B * T, H), self.w_ih, B * T, 8 * H, H, True, True, out_dtype=torch.float32, bias=self.b_ih).view(B, T, 8 * H)
        seq = torch.empty((B, T, H), dtype=dt, device=self.dev)
        _, hn, cn = F.tft_lstm_fwd(xp[:, :enc, :4 * H], self.w_hh[0], ch, cc, out=seq[:, :enc])
        F.tft_lstm_fwd(xp[:, enc:, 4 * H:], self.w_hh[1], hn, cn, out=seq[:, enc:])
        # gate + skip, enrichment, attention of the decoder positions, and the decoder's three stages
        temporal = F.tft_grn_fwd(seq.view(B * T, H), self.input_gate, res=feat.view(B * T, H), eps=LN_EPS)
        enriched = F.tft_grn_fwd(temporal, self.enrichment, ctx=ce, rows_per_ctx=T, eps=LN_EPS)
        qkv = F.gemm(enriched, self.w_qkv, B * T, 288, H, True, True)
        r = F.tft_attention_fwd(qkv, self.w_o, B, T, enc, want_probs=explain)
        att, probs = (r if explain else (r, None))
        x = F.tft_grn_fwd(att.view(B * nq, H), self.attention_gate, res=enriched.view(B, T, H), res_rows_per_batch=nq, eps=LN_EPS)
        x = F.tft_grn_fwd(x, self.positionwise, eps=LN_EPS)
        q = F.tft_grn_fwd(x, self.decoder_gate, res=temporal.view(B, T, H), res_rows_per_batch=nq, wq=self.wq, bq=self.bq,
                          want_out=False, eps=LN_EPS)
        out = q.view(B, nq, -1)
        return (out, hist_w, fut_w, probs) if explain else out
