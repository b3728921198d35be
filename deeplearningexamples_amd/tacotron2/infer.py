"""Tacotron2 inference on the gfx950 library: text -> mel spectrogram, Tacotron2.infer of SpeechSynthesis/Tacotron2/tacotron2/
model.py:678-691 (embedding, Encoder.infer, Decoder.infer :515-595, postnet + residual).

The encoder (eval-mode BatchNorm, no dropout, packed bi-LSTM), the LSTMCell-as-GEMM-epilogue, the location-sensitive attention
step and the eval-mode postnet are the launches of tacotron2/engine.py.  What is new is the free-running decoder loop:
  * per step: [dle_t2_prenet_infer] -> attention LSTMCell (dle_t2_lstm_gemm_fwd over ONE [4 Ha, P + E + Ha] weight) -> query GEMM ->
    dle_t2_attention_fwd (location term fused) -> decoder LSTMCell -> dle_t2_frame_infer (mel frame, gate logit, the stop
    bookkeeping of model.py:578-582 and the step counter, on the device);
  * the recurrent state lives in two alternating operand buffers (even / odd step): every kernel writes its result straight
    into the operand of the launch that consumes it;
  * K steps (K even) are captured once per (B, Ti) as ONE linear HIP graph and replayed; the host reads the stop flag once per
    chunk, and whatever was computed after the stop is cut off at n_steps;
  * output placement: the mel frames and gate logits go through the DEVICE step word (kernel pointer arguments are frozen in a
    captured graph, the word is not); the attention kernel, whose behaviour is not touched, writes its weights into a K-step
    staging buffer that is appended to the alignments between replays;
  * the prenet's dropout stays on (model.py:129): its masks follow the contract in include/dle_mi355x.h -- (seed, offset
    1 + 2 t + l) with t read from the same device word, so a replay draws fresh masks and a seed fixes the spectrogram.
The 16-bit operands are prepared ONCE (refresh() after the model's weights change), one set of work buffers per (B, Ti) serves every
call.  Restrictions: B <= 8, n_frames_per_step = 1, attention_dim % 32 == 0 and an odd location kernel (the fused location term).
No CPU path.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from ..waveglow import ops as wops
from . import ops
from .model import Tacotron2

NPAD = 8
DEFAULT_CHUNK = 16        # steps per captured graph: see DESIGN.md 4e-2 for the measurement behind it
MAX_BATCH = 8


class Tacotron2Synthesizer:
    def __init__(self, model: Tacotron2, compute_dtype=torch.float16, max_decoder_steps=2000, gate_threshold=0.5,
                 early_stopping=True, seed=1234, chunk=DEFAULT_CHUNK, graph=True, fused_tail=False):
        """chunk: decoder steps per graph replay / per host check of the stop flag (even); graph=False launches the same chain
        eagerly; fused_tail: the frame and the next step's prenet as ONE one-workgroup launch instead of two."""
        self.model, self.cfg = model, model.cfg
        self.dev = model.store.flat.device
        self.dtype = compute_dtype
        self.max_decoder_steps, self.gate_threshold = int(max_decoder_steps), float(gate_threshold)
        self.early_stopping, self.seed = bool(early_stopping), int(seed)
        self.chunk, self.graph, self.fused_tail = int(chunk), bool(graph), bool(fused_tail)
        if self.chunk < 2 or self.chunk % 2:
            raise ValueError("chunk must be even: the operand buffers alternate with the step's parity")
        if self.max_decoder_steps < 1:
            raise ValueError("max_decoder_steps must be positive")
        c = self.cfg
        self.E, self.A, self.Ha, self.Hd, self.P = (c["encoder_embedding_dim"], c["attention_dim"], c["attention_rnn_dim"],
                                                    c["decoder_rnn_dim"], c["prenet_dim"])
        self.NM, self.NF, self.KL = c["n_mel_channels"], c["attention_location_n_filters"], c["attention_location_kernel_size"]
        self.h = self.E // 2
        self.NO = (self.NM + 1 + NPAD - 1) // NPAD * NPAD
        for v in (self.E, self.A, self.Ha, self.Hd, self.P, self.NM, self.NF, self.h, c["postnet_embedding_dim"]):
            if v % 8:
                raise ValueError("every layer width must be a multiple of 8")
        if self.A % 32 or self.KL % 2 == 0:
            raise ValueError("the fused location term needs attention_dim % 32 == 0 and an odd location kernel size")
        self.p = model.store
        self._buf = dict(model.named_buffers())
        self._buffers = {}
        self.gate_outputs = None
        self.time_decoder, self.decoder_ms = False, None   # tools/tacotron2_infer_perf.py: event-timed decoder loop of the last call
        self.refresh()

    # ------------------------------------------------------------------ operands
    def _z(self, *shape, dtype=None):
        return torch.zeros(shape, dtype=dtype or self.dtype, device=self.dev)

    def _e(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.dev)

    def _cast(self, t):
        return F.cast(t, self.dtype)

    def _conv_w(self, name):
        w = self.p[name]
        w16 = self._e(w.shape[0], w.shape[2] * w.shape[1])
        wops.weight_norm_fwd(w, None, w16)
        return w16

    def _sum2(self, a, b):
        out = torch.empty_like(a)
        F.axpby_(a, b, out, 1.0, 1.0)
        return out

    def refresh(self):
        """fp32 parameters -> the 16-bit operands of every launch: at construction, and again after the model's weights change.
        A captured graph holds these buffers by address, so they are rewritten in place once they exist."""
        p, dt = self.p, self.dtype
        E, A, Ha, Hd, P, NM = self.E, self.A, self.Ha, self.Hd, self.P, self.NM
        w = {}
        w["emb"] = self._cast(p["embedding.weight"])
        for i in range(self.cfg["encoder_n_convolutions"]):
            w["enc%d" % i] = self._conv_w("encoder.convolutions.%d.0.conv.weight" % i)
        for sfx in ("", "_reverse"):
            w["eih" + sfx] = self._cast(p["encoder.lstm.weight_ih_l0" + sfx])
            w["ehh" + sfx] = self._cast(p["encoder.lstm.weight_hh_l0" + sfx])
            w["eb" + sfx] = self._sum2(p["encoder.lstm.bias_ih_l0" + sfx], p["encoder.lstm.bias_hh_l0" + sfx])
        w["pre0"] = self._cast(p["decoder.prenet.layers.0.linear_layer.weight"])
        w["pre1"] = self._cast(p["decoder.prenet.layers.1.linear_layer.weight"])
        # attention LSTM: ONE [4 Ha, P + E + Ha] operand over [prenet | context | attention_hidden], the two biases summed
        w["a_full"] = self._e(4 * Ha, P + E + Ha)
        F.cast_rows(p["decoder.attention_rnn.weight_ih"], dt, out=w["a_full"][:, :P + E])
        F.cast_rows(p["decoder.attention_rnn.weight_hh"], dt, out=w["a_full"][:, P + E:])
        w["a_b"] = self._sum2(p["decoder.attention_rnn.bias_ih"], p["decoder.attention_rnn.bias_hh"])
        w["d_cat"] = self._e(4 * Hd, Ha + E + Hd)
        F.cast_rows(p["decoder.decoder_rnn.weight_ih"], dt, out=w["d_cat"][:, :Ha + E])
        F.cast_rows(p["decoder.decoder_rnn.weight_hh"], dt, out=w["d_cat"][:, Ha + E:])
        w["d_b"] = self._sum2(p["decoder.decoder_rnn.bias_ih"], p["decoder.decoder_rnn.bias_hh"])
        att = "decoder.attention_layer."
        w["q"] = self._cast(p[att + "query_layer.linear_layer.weight"])
        w["mem"] = self._cast(p[att + "memory_layer.linear_layer.weight"])
        w["v"] = p[att + "v.linear_layer.weight"].view(-1)
        # location conv [F, 2, KL] and dense [A, F] pre-multiplied, then the compact k = tap * 2 + channel form (engine.py)
        loc_c = self._z(self.NF, self.KL * 8)
        wops.weight_norm_fwd(p[att + "location_layer.location_conv.conv.weight"], None, loc_c, cip=8)
        loc_d = self._cast(p[att + "location_layer.location_dense.linear_layer.weight"])
        loc = F.gemm(loc_d, loc_c, A, self.KL * 8, self.NF, True, False)
        kk = (2 * self.KL + 31) // 32 * 32
        w["loc2"] = self._z(A, kk)
        w["loc2"][:, :2 * self.KL].view(A, self.KL, 2).copy_(loc.view(A, self.KL, 8)[:, :, :2])
        w["proj"] = self._z(self.NO, Hd + E)
        F.cast_rows(p["decoder.linear_projection.linear_layer.weight"], dt, out=w["proj"][:NM])
        F.cast_rows(p["decoder.gate_layer.linear_layer.weight"], dt, out=w["proj"][NM:NM + 1])
        w["proj_b"] = self._z(self.NO, dtype=torch.float32)
        w["proj_b"][:NM].copy_(p["decoder.linear_projection.linear_layer.bias"])
        w["proj_b"][NM:NM + 1].copy_(p["decoder.gate_layer.linear_layer.bias"])
        for i in range(self.cfg["postnet_n_convolutions"]):
            w["post%d" % i] = self._conv_w("postnet.convolutions.%d.0.conv.weight" % i)
        for name, buf in self._buf.items():
            if name.endswith("running_var"):
                w["rstd." + name[:-12]] = torch.rsqrt(buf + 1e-5)
        old = getattr(self, "w", None)
        if old is None:
            self.w = w
        else:
            for k, t in w.items():
                old[k].copy_(t)

    def _conv_bn(self, x, b, t, name, w16, act):
        """Conv1d(k, pad (k-1)/2) + BatchNorm1d(eval: running statistics) + act on rows (b, t); no dropout in eval mode."""
        wt = self.p[name + ".0.conv.weight"]
        k, cout = wt.shape[2], wt.shape[0]
        col = wops.taps(x, b, t, k, 1, k // 2)
        pre = F.gemm(col, w16, b * t, cout, col.shape[1], True, True, bias=self.p[name + ".0.conv.bias"])
        bn = name + ".1"
        y, _ = F.bn_fwd_apply(pre, self._buf[bn + ".running_mean"], self.w["rstd." + bn], self.p[bn + ".weight"], self.p[bn + ".bias"],
                              relu=(act == "relu"))
        return ops.tanh_fwd(y) if act == "tanh" else y

    # ------------------------------------------------------------------ buffers of one (B, Ti)
    def _work(self, b, ti):
        key = (b, ti)
        wk = self._buffers.get(key)
        if wk is None:
            E, A, Ha, Hd, P, NM, K = self.E, self.A, self.Ha, self.Hd, self.P, self.NM, self.chunk
            f32, i32 = torch.float32, torch.int32
            rows = (self.max_decoder_steps + K - 1) // K * K
            wk = dict(memory=self._z(b * ti, E), pm=self._e(b * ti, A), lengths=torch.zeros(b, dtype=torch.int64, device=self.dev),
                      x_a=self._z(2, b, P + E + Ha),                 # [prenet | context_{t-1} | attention_hidden_{t-1}]
                      x_d=self._z(2, b, Ha + E + Hd),                # [attention_hidden_t | context_t | decoder_hidden_{t-1}]
                      hc=self._z(b, Hd + E),                         # [decoder_hidden_t | context_t]
                      ac=self._z(2, b, Ha, dtype=f32), dc=self._z(2, b, Hd, dtype=f32),
                      ga=self._e(b, 4 * Ha), gd=self._e(b, 4 * Hd), q=self._e(b, A, dtype=f32),
                      awc=self._z(2, b * ti, 8), tanh=self._e(b * ti, A),          # ONE scratch for the tanh the kernel insists on
                      aw_stage=self._z(K, b, ti, dtype=f32), frame=self._z(b, NM, dtype=f32),
                      state=torch.zeros(4, dtype=torch.int64, device=self.dev),
                      nf=torch.ones(b, dtype=i32, device=self.dev), ml=torch.zeros(b, dtype=i32, device=self.dev),
                      mel=self._z(b, self.max_decoder_steps, NM, dtype=f32), gate=self._z(b, self.max_decoder_steps, dtype=f32),
                      aligns=self._z(rows, b, ti, dtype=f32), graph=None)
            self._buffers[key] = wk
        return wk

    def _reset(self, wk):
        """The state Decoder.infer starts from (get_go_frame, initialize_decoder_states, model.py:527-540)."""
        for k in ("x_a", "x_d", "hc", "ac", "dc", "awc", "frame", "state", "ml"):
            wk[k].zero_()
        wk["nf"].fill_(1)
        if self.fused_tail:            # the first step's prenet has no frame launch in front of it
            ops.prenet_infer(None, self.w["pre0"], self.w["pre1"], wk["x_a"][0][:, :self.P], self.seed, wk["state"])

    def _step(self, wk, k, b):
        """Decoder step at position k of a chunk; chunks start at even steps, so k & 1 is the step's parity."""
        E, A, Ha, Hd, P = self.E, self.A, self.Ha, self.Hd, self.P
        w, par = self.w, k & 1
        xa, xd, xa_n, xd_n = wk["x_a"][par], wk["x_d"][par], wk["x_a"][1 - par], wk["x_d"][1 - par]
        if not self.fused_tail:
            ops.prenet_infer(wk["frame"], w["pre0"], w["pre1"], xa[:, :P], self.seed, wk["state"][par:])
        ops.lstm_gemm_fwd(xa, w["a_full"], w["a_b"], None, wk["ac"][par], wk["ac"][1 - par], wk["ga"], [xd[:, :Ha], xa_n[:, P + E:]])
        F.gemm(xd[:, :Ha], w["q"], b, A, Ha, True, True, out=wk["q"])
        ops.attention_fwd(wk["q"], wk["pm"], w["v"], wk["memory"], wk["lengths"], wk["awc"][par], wk["tanh"], wk["aw_stage"][k],
                          wk["awc"][1 - par], [xd[:, Ha:Ha + E], xa_n[:, P:P + E], wk["hc"][:, Hd:]], wloc=w["loc2"], kl=self.KL)
        ops.lstm_gemm_fwd(xd, w["d_cat"], w["d_b"], None, wk["dc"][par], wk["dc"][1 - par], wk["gd"], [xd_n[:, Ha + E:], wk["hc"][:, :Hd]])
        ops.frame_infer(wk["hc"], w["proj"], w["proj_b"], wk["mel"], wk["gate"], wk["frame"], wk["nf"], wk["ml"], wk["state"], par,
                        self.gate_threshold, self.max_decoder_steps,
                        prenet=(w["pre0"], w["pre1"], xa_n[:, :P]) if self.fused_tail else None, seed=self.seed)

    def _chunk(self, wk, b):
        for k in range(self.chunk):
            self._step(wk, k, b)

    def _capture(self, wk, b):
        """One eager chunk (loads every kernel outside the capture), then the chunk as ONE linear graph.  The state the warm-up
        leaves behind is reset by the caller."""
        self._chunk(wk, b)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._chunk(wk, b)
        wk["graph"] = g

    # ------------------------------------------------------------------ the call
    @torch.no_grad()
    def infer(self, text, text_lengths):
        """text int64 [B, Ti] (sorted by length, descending, 0-padded), text_lengths int64 [B] ->
        (mel_outputs_postnet fp32 [B, n_mel, T], mel_lengths int32 [B], alignments fp32 [B, T, Ti]), T = n_steps.
        The gate logits fp32 [B, T] of the call are left in self.gate_outputs."""
        C.require_cuda(text, text_lengths)
        if text.dim() != 2 or text_lengths.dim() != 1 or text_lengths.numel() != text.shape[0]:
            raise ValueError("text [B, Ti] and text_lengths [B]")
        b, ti = text.shape
        if b > MAX_BATCH:
            raise ValueError("the decoder-step kernels hold at most %d rows (got a batch of %d)" % (MAX_BATCH, b))
        E, A, NM, h, dt, cfg, w = self.E, self.A, self.NM, self.h, self.dtype, self.cfg, self.w
        wk = self._work(b, ti)
        text_lengths = text_lengths.to(torch.int64)
        wk["lengths"].copy_(text_lengths)
        # ---- encoder (Encoder.infer, model.py:218-252): embedding, 3 x (conv + BN + ReLU), bi-LSTM over the packed batch
        x = F.rows_gather(w["emb"], text.reshape(-1).contiguous())
        for i in range(cfg["encoder_n_convolutions"]):
            x = self._conv_bn(x, b, ti, "encoder.convolutions.%d" % i, w["enc%d" % i], "relu")
        memory = wk["memory"]
        memory.zero_()
        mem3 = memory.view(b, ti, E)
        live_all = (torch.arange(ti, device=self.dev)[:, None] < text_lengths[None, :]).to(torch.float32).contiguous()   # [Ti, B]
        for d, sfx in enumerate(("", "_reverse")):
            gx = F.gemm(x, w["eih" + sfx], b * ti, 4 * h, E, True, True, bias=w["eb" + sfx]).view(b, ti, 4 * h)
            gates = self._e(b, ti, 4 * h)                               # rows (b, t) like gx: the addend shares the output's pitch
            hs = self._z(2, b, h)
            cs = self._z(2, b, h, dtype=torch.float32)
            for k, t in enumerate(range(ti - 1, -1, -1) if d else range(ti)):
                cur = k & 1
                F.gemm(hs[cur], w["ehh" + sfx], b, 4 * h, h, True, True, out=gates[:, t], act=C.ACT_ADD, mask_src=gx[:, t])
                ops.lstm_fwd(gates[:, t], cs[cur], cs[1 - cur], [hs[1 - cur]], live=live_all[t], h_prev=hs[cur],
                             out_dst=mem3[:, t, d * h:(d + 1) * h])
        F.gemm(memory, w["mem"], b * ti, A, E, True, True, out=wk["pm"])
        # ---- decoder (Decoder.infer)
        use_graph = self.graph
        if use_graph and wk["graph"] is None:
            self._reset(wk)
            self._capture(wk, b)
        self._reset(wk)
        if self.time_decoder:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        K, steps, done = self.chunk, 0, False
        while steps < self.max_decoder_steps:
            if use_graph:
                wk["graph"].replay()
            else:
                self._chunk(wk, b)
            wk["aligns"][steps:steps + K].copy_(wk["aw_stage"])
            steps += K
            if self.early_stopping and int(wk["state"][3].item()):      # ONE host read per chunk
                done = True
                break
        n = int(wk["state"][2].item()) if done else self.max_decoder_steps
        if self.time_decoder:
            ev[1].record()
            ev[1].synchronize()
            self.decoder_ms = ev[0].elapsed_time(ev[1])
        if n == self.max_decoder_steps and not (self.early_stopping and int(wk["state"][3].item())):
            print("Warning! Reached max decoder steps")
        # ---- postnet (eval) + residual on the first n frames
        mel = wk["mel"][:, :n].contiguous()                              # [B, n, n_mel] fp32: rows (b, t)
        y = F.cast_rows(mel.view(b * n, NM), dt)
        npc = cfg["postnet_n_convolutions"]
        for i in range(npc):
            y = self._conv_bn(y, b, n, "postnet.convolutions.%d" % i, w["post%d" % i], "tanh" if i < npc - 1 else "none")
        post = (mel + y.float().view(b, n, NM)).permute(0, 2, 1).contiguous()
        self.gate_outputs = wk["gate"][:, :n].clone()
        return post, wk["ml"].clone(), wk["aligns"][:n].permute(1, 0, 2).contiguous()
