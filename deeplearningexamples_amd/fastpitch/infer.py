"""FastPitch inference on the gfx950 library: symbol ids -> mel spectrogram, FastPitch.infer of
SpeechSynthesis/FastPitch/fastpitch/model.py:327-385 with the FFTransformer of transformer.py:168-213.

Layout and contract.  Activations are 16-bit, channels-last and PACKED: [total_rows, C] with a device int32 cu_seqlens[B + 1], as
in BertPredictor; there are no padding rows and no masks, and every kernel reads rows outside a row's own utterance as zero.  The
reference's BATCHED result is not reproduced on purpose: it zeroes the padded positions in front of each convolution, the
convolution then writes relu(bias + w x[len - 1]) into the first padding row, and the next convolution reads that value at the
utterance's last real position -- so its output for an utterance depends on what shares the batch.  Here EVERY UTTERANCE GETS
WHAT THE REFERENCE GIVES IT WHEN IT IS RUN ALONE (batch 1), whatever else is in the batch (tests/golden/fastpitch_infer.npz is
generated that way; tests/test_gpu_fastpitch_infer.py checks a batch of 3 against three batch-1 runs).

Launches.  Embedding: dle_fp_embed (word + positional (+ speaker), the positional table built once on the host).  Per FFT layer 7:
qkv dle_gemm with bias; dle_attention_fwd_varlen (scale d_head^-0.5); o_net dle_gemm; dle_layernorm_fwd(x, residual);
dle_conv1d_packed_fwd; dle_conv1d_packed_fwd with slope 0 (the ReLU between the two); dle_layernorm_fwd(x, residual).  A
temporal predictor of n layers: n x (dle_conv1d_packed_fwd, dle_fp_relu_layernorm_fwd), the last with the fc folded in.  Then, in
this order: duration and pitch predictors -> pitch_emb (dle_fp_scalar_conv_add, in place) (-> energy predictor -> energy_emb) ->
dle_fp_durations -> dle_fp_expand (the length regulator as a gather + the decoder's positional embedding) -> decoder -> proj
(dle_gemm) -> dle_fp_unpack_mel (fp32 [B, n_mel, T_max], padding frames = proj.bias, as the reference's are).

Host synchronisation.  Exactly ONE device-to-host read per batch: cu_out, the predicted frame counts, which size the decoder's
buffers and the output (the same copy carries the flag of the id check).  `d2h_reads` counts them.  There is no graph capture:
the shapes of everything behind the length regulator depend on the predicted lengths.

Not built (one-line errors): d_head != 64, pitch_conditioning_formants != 1, pre_lnorm, an id equal to padding_idx inside a text,
a text or a predicted spectrogram longer than 1024 rows (the envelope of the packed attention kernel), fp32.  No CPU path.
"""
import numpy as np
import torch

from .. import functional as F
from ..utils.frontend import gpu_device, require_16bit
from .model import LJSPEECH_PITCH, LN_EPS, MAX_ROWS, FastPitchModel, check_config, normalize_keys, positional_table


class _FFTLayer:
    __slots__ = ("qkv", "qkv_b", "o", "ln1", "c1", "c1_b", "c2", "c2_b", "ln2")


class _Predictor:
    __slots__ = ("convs", "fc_w", "fc_b")


class FastPitchSynthesizer:
    def __init__(self, model_or_state, config=None, dtype=torch.float16, device=None):
        """model_or_state: a FastPitchModel (left untouched) or the reference's state dict (then `config` holds the reference's
        config keys; missing ones take the defaults of fastpitch/arg_parser.py).  dtype: torch.float16 or torch.bfloat16."""
        require_16bit(dtype, "FastPitchSynthesizer")
        if isinstance(model_or_state, FastPitchModel):
            model = model_or_state
        else:
            model = FastPitchModel(config or {}, device="cpu").load_state_dict(model_or_state)
        self.cfg = cfg = check_config(model.cfg)
        for k in ("in_fft_d_head", "out_fft_d_head"):
            if cfg[k] != 64:
                raise ValueError("%s = %d: the packed attention kernel is built for 64-wide heads only" % (k, cfg[k]))
        if cfg["pitch_conditioning_formants"] != 1:
            raise ValueError("pitch_conditioning_formants = %d: only 1 is built" % cfg["pitch_conditioning_formants"])
        if cfg.get("pre_lnorm"):
            raise ValueError("pre_lnorm: the pre-LayerNorm variant of the FFT block is not built")
        self.dev = dev = gpu_device(device, "FastPitchSynthesizer")
        self.dtype = dtype
        self.d = d = cfg["symbols_embedding_dim"]
        self.n_mel = cfg["n_mel_channels"]
        P = model.params
        f32 = lambda k: P[k].detach().float().contiguous().to(dev)
        w16 = lambda k: P[k].detach().float().to(dtype).contiguous().to(dev)
        conv16 = lambda k: F.pack_conv1d_weight(P[k].detach().float(), dtype).to(dev)

        def fft(pre, n_layers):
            out = []
            for n in range(n_layers):
                p, l = "%slayers.%d." % (pre, n), _FFTLayer()
                l.qkv, l.qkv_b, l.o = w16(p + "dec_attn.qkv_net.weight"), f32(p + "dec_attn.qkv_net.bias"), w16(p + "dec_attn.o_net.weight")
                l.ln1 = (f32(p + "dec_attn.layer_norm.weight"), f32(p + "dec_attn.layer_norm.bias"))
                l.c1, l.c1_b = conv16(p + "pos_ff.CoreNet.0.weight"), f32(p + "pos_ff.CoreNet.0.bias")
                l.c2, l.c2_b = conv16(p + "pos_ff.CoreNet.2.weight"), f32(p + "pos_ff.CoreNet.2.bias")
                l.ln2 = (f32(p + "pos_ff.layer_norm.weight"), f32(p + "pos_ff.layer_norm.bias"))
                out.append(l)
            return out

        def predictor(pre, n_layers):
            pr = _Predictor()
            pr.convs = []
            for n in range(n_layers):
                p = "%slayers.%d." % (pre, n)
                pr.convs.append((conv16(p + "conv.weight"), f32(p + "conv.bias"), f32(p + "norm.weight"), f32(p + "norm.bias")))
            pr.fc_w, pr.fc_b = f32(pre + "fc.weight"), f32(pre + "fc.bias")
            return pr

        with torch.no_grad():
            self.word = f32("encoder.word_emb.weight")
            self.pos = positional_table(MAX_ROWS, d).float().contiguous().to(dev)       # both FFTransformers have d_model = d
            self.enc, self.dec = fft("encoder.", cfg["in_fft_n_layers"]), fft("decoder.", cfg["out_fft_n_layers"])
            self.enc_heads, self.dec_heads = cfg["in_fft_n_heads"], cfg["out_fft_n_heads"]
            self.dur_p = predictor("duration_predictor.", cfg["dur_predictor_n_layers"])
            self.pitch_p = predictor("pitch_predictor.", cfg["pitch_predictor_n_layers"])
            self.pitch_w, self.pitch_b = f32("pitch_emb.weight").reshape(d, -1).contiguous(), f32("pitch_emb.bias")
            self.energy = bool(cfg["energy_conditioning"])
            if self.energy:
                self.energy_p = predictor("energy_predictor.", cfg["energy_predictor_n_layers"])
                self.energy_w, self.energy_b = f32("energy_emb.weight").reshape(d, -1).contiguous(), f32("energy_emb.bias")
            # fp32 speaker rows already scaled by speaker_emb_weight (model.py:336-337), one per speaker
            self.spk = (f32("speaker_emb.weight") * float(cfg["speaker_emb_weight"])).contiguous() if cfg["n_speakers"] > 1 else None
            self.proj, self.proj_b = w16("proj.weight"), f32("proj.bias")
            mean, std = float(P["pitch_mean"][0]), float(P["pitch_std"][0])
            self.pitch_stats = LJSPEECH_PITCH if std == 0.0 else (mean, std)           # model.py:350-354
        self.d2h_reads = 0          # device-to-host copies made by infer() so far: one per batch
        self.last = {}              # reps, tok_start, cu_in, cu_out of the most recent batch (device tensors; tests and tools)

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, ema=False, **kw):
        """The reference's checkpoint file (or the dict it holds): {'state_dict', 'config', 'train_setup', ...}.  The reference's
        loader (models.py:256) reads 'state_dict'; ema=True takes 'ema_state_dict', the name its trainer saves the averaged weights
        under (common/utils.py:299), and fails when the checkpoint holds none."""
        ckpt = path_or_ckpt
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        key = "ema_state_dict" if ema else "state_dict"
        if ckpt.get(key) is None:
            raise KeyError("not a FastPitch checkpoint with %s weights: no %r entry" % ("EMA" if ema else "model", key))
        return cls(normalize_keys(ckpt[key]), config=ckpt.get("config") or {}, **kw)

    # ------------------------------------------------------------------ pieces
    def _fft(self, x, layers, heads, cu, max_len, total):
        d, dt = self.d, self.dtype
        h = heads * 64
        for l in layers:
            qkv = F.gemm(x, l.qkv, total, 3 * h, d, True, True, bias=l.qkv_b)
            ctx = F.attention_fwd_varlen(qkv, cu, max_len, heads, 64 ** -0.5)
            ao = F.gemm(ctx, l.o, total, d, h, True, True)
            x1 = F.layernorm_fwd(ao, l.ln1[0], l.ln1[1], residual=x, eps=LN_EPS, write_z=False)[0]
            t = F.conv1d_packed_fwd(x1, l.c1, l.c1_b, cu, max_len)
            o2 = F.conv1d_packed_fwd(t, l.c2, l.c2_b, cu, max_len, slope=0.0)
            x = F.layernorm_fwd(o2, l.ln2[0], l.ln2[1], residual=x1, eps=LN_EPS, write_z=False)[0]
        return x

    def _predict(self, x, pr, cu, max_len):
        """TemporalPredictor (model.py:90-109) on packed rows -> fp32 [total] (n_predictions = 1)."""
        n = len(pr.convs)
        for i, (w, b, g, be) in enumerate(pr.convs):
            t = F.conv1d_packed_fwd(x, w, b, cu, max_len)
            if i < n - 1:
                x = F.fp_relu_layernorm_fwd(t, g, be, eps=LN_EPS)[0]
            else:
                return F.fp_relu_layernorm_fwd(t, g, be, eps=LN_EPS, fc_w=pr.fc_w, fc_b=pr.fc_b, want_y=False)[1].reshape(-1)

    def _pack(self, padded, rows):
        """[B, L] (or [B, 1, L]) fp32 values of the caller -> packed fp32 [total] on the device."""
        b, l = len(self._lens), self._lmax
        t = torch.as_tensor(padded).to(self.dev, torch.float32).reshape(b, -1)
        if t.shape[1] < l:
            raise ValueError("a per-token override must cover %d tokens (got %d)" % (l, t.shape[1]))
        return t[:, :l].reshape(-1)[rows].contiguous()

    # ------------------------------------------------------------------ the forward pass
    def infer(self, texts, pace=1.0, dur_tgt=None, pitch_tgt=None, energy_tgt=None, pitch_transform=None, max_duration=75,
              speaker=0, text_lens=None):
        """texts: a list of 1-D id tensors, or a padded [B, L] tensor with text_lens (a list or a host tensor; a device tensor
        costs one more device-to-host read).  The overrides are the reference's: dur_tgt [B, L], pitch_tgt [B, 1, L], energy_tgt
        [B, 1, L], pitch_transform(pitch [B, 1, L] fp32, lens [B], mean, std) applied in torch.
        -> (mel fp32 [B, n_mel, T_max] with padding frames = proj.bias, mel_lens int64 [B], dur_pred fp32 [B, L], pitch_pred fp32
        [B, 1, L], energy_pred fp32 [B, L] or None), per-token outputs zero padded -- each utterance as the reference computes
        it at batch 1."""
        dev, dt, d = self.dev, self.dtype, self.d
        if isinstance(texts, torch.Tensor) and texts.dim() == 2:
            if text_lens is None:
                raise ValueError("a padded [B, L] text tensor needs text_lens")
            if isinstance(text_lens, torch.Tensor) and text_lens.is_cuda:
                self.d2h_reads += 1
            lens = [int(n) for n in (text_lens.tolist() if isinstance(text_lens, torch.Tensor) else text_lens)]
            if len(lens) != texts.shape[0] or (lens and max(lens) > texts.shape[1]):
                raise ValueError("text_lens does not fit the [B, L] text tensor")
            texts = [texts[i, :n] for i, n in enumerate(lens)]
        texts = [torch.as_tensor(t) for t in texts]
        if not texts or any(t.dim() != 1 or t.dtype not in (torch.int64, torch.int32) for t in texts):
            raise ValueError("texts must be a non-empty list of 1-D integer id tensors")
        lens = [int(t.numel()) for t in texts]
        for i, n in enumerate(lens):
            if n < 1:
                raise ValueError("utterance %d is empty" % i)
            if n > MAX_ROWS:
                raise ValueError("utterance %d has %d symbols: texts longer than %d rows are not built (the packed attention "
                                 "kernel's envelope)" % (i, n, MAX_ROWS))
        if not (float(pace) > 0.0):
            raise ValueError("pace must be positive (got %r)" % (pace,))
        if self.spk is not None and not 0 <= int(speaker) < self.spk.shape[0]:
            raise ValueError("speaker %r outside the %d speakers of the model" % (speaker, self.spk.shape[0]))
        b, lmax, total = len(lens), max(lens), sum(lens)
        self._lens, self._lmax = lens, lmax
        with torch.no_grad():
            ids = torch.cat([t.to(dev, torch.int64) for t in texts]).contiguous()
            bad = ((ids == self.cfg["padding_idx"]) | (ids < 0) | (ids >= self.word.shape[0])).any().to(torch.int32).reshape(1)
            cu_host = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            cu = torch.from_numpy(cu_host).to(dev)
            # flat [B * L] index of every packed row (host arithmetic on the known lengths: no synchronisation)
            rows = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int64) + i * lmax for i, n in enumerate(lens)])).to(dev)

            def pad(packed, fill_shape):
                out = torch.zeros((b * lmax,), dtype=torch.float32, device=dev)
                out[rows] = packed
                return out.view(fill_shape)

            spk = self.spk[int(speaker)] if self.spk is not None else None
            x = F.fp_embed(ids, self.word, self.pos, cu, lmax, dt, spk=spk)
            enc = self._fft(x, self.enc, self.enc_heads, cu, lmax, total)
            log_dur = self._predict(enc, self.dur_p, cu, lmax)
            pitch = self._predict(enc, self.pitch_p, cu, lmax)
            pitch_pred = pad(pitch, (b, 1, lmax))
            if pitch_transform is not None:
                mean, std = self.pitch_stats
                pitch = pitch_transform(pitch_pred, torch.tensor(lens, device=dev), mean, std).to(torch.float32).reshape(-1)[rows].contiguous()
                pitch_pred = pad(pitch, (b, 1, lmax))                    # (a shift moves the reference's padding too; here it stays zero)
            F.fp_scalar_conv_add_(enc, pitch if pitch_tgt is None else self._pack(pitch_tgt, rows), self.pitch_w, self.pitch_b, cu, lmax)
            energy_pred = None
            if self.energy:
                if energy_tgt is None:
                    energy = self._predict(enc, self.energy_p, cu, lmax)
                    energy_pred = pad(energy, (b, lmax))
                else:
                    energy = self._pack(energy_tgt, rows)
                F.fp_scalar_conv_add_(enc, energy, self.energy_w, self.energy_b, cu, lmax)
            # the frame counts are NOT cut at 1024 here: a longer prediction is reported below, by utterance and length
            dur, reps, tok_start, cu_out = F.fp_durations(log_dur, cu, lmax, pace=pace, max_duration=max_duration, max_out=1 << 30)
            if dur_tgt is not None:
                _, reps, tok_start, cu_out = F.fp_durations(self._pack(dur_tgt, rows), cu, lmax, pace=pace, from_log=False,
                                                            max_out=1 << 30)
            dur_pred = pad(dur, (b, lmax))
            host = torch.cat([cu_out, bad]).cpu().tolist()                  # the batch's one device-to-host read
            self.d2h_reads += 1
            if host[-1]:
                raise ValueError("a text holds an id equal to padding_idx (%d) or outside the %d symbols: padding inside a text "
                                 "is not built" % (self.cfg["padding_idx"], self.word.shape[0]))
            out_lens = [host[i + 1] - host[i] for i in range(b)]
            for i, n in enumerate(out_lens):
                if n > MAX_ROWS:
                    raise ValueError("utterance %d: predicted spectrogram of %d frames; more than %d rows are not built (the packed "
                                     "attention kernel's envelope)" % (i, n, MAX_ROWS))
            self.last = dict(reps=reps, tok_start=tok_start, cu_in=cu, cu_out=cu_out)
            total_out, tmax = host[b], max(out_lens)
            mel_lens = (cu_out[1:] - cu_out[:-1]).to(torch.int64)
            if total_out == 0:
                return torch.empty((b, self.n_mel, 0), dtype=torch.float32, device=dev), mel_lens, dur_pred, pitch_pred, energy_pred
            y = F.fp_expand(enc, self.pos, reps, tok_start, cu, cu_out, lmax, tmax, total_out)
            y = self._fft(y, self.dec, self.dec_heads, cu_out, tmax, total_out)
            mel16 = F.gemm(y, self.proj, total_out, self.n_mel, d, True, True, bias=self.proj_b)
            mel = F.fp_unpack_mel(mel16, self.proj_b, cu_out, tmax)
        return mel, mel_lens, dur_pred, pitch_pred, energy_pred

    __call__ = infer
