"""Jasper inference on the gfx950 library: log-mel features -> log-probabilities / transcripts, the forward of
SpeechRecognition/Jasper/jasper/model.py:239-251 (Jasper.forward with use_conv_masks) behind the front end of
common/features.py and the leading pad of inference.py:329-333, in front of GreedyCTCDecoder and common/helpers.py's
ctc_decoder_predictions_tensor.

Layout.  Activations are 16-bit, channels-last and PACKED: [total_rows, C] with device int32 cu tables; there are no padding rows.
Every utterance is computed as the reference computes it at batch size 1: with masked convolutions that is what the reference gives
it in any batch, except that the reference also decodes the frames behind an utterance's length, which this does not copy.

Launches, for S sub-blocks in all and P residual panes in all (10x5dr: 53 and 1 + 2 + ... + 10 = 55):
  1   dle_qn_normalize_pack_lead     per-feature normalisation, mask, transpose, 16-bit cast, `pad_leading` zero rows in front
  S   dle_conv1d_bn_packed_fwd       dense conv + BatchNorm (+ the block's residual sum) + ReLU, one launch per sub-block
  P   dle_conv2d_fwd_affine          the residual panes of a block (1x1 conv + BatchNorm over [1, 1, rows, C]), computed FIRST and
                                     chained through the `residual` operand into a running sum, which the block's last sub-block
                                     consumes; every link of the chain is rounded to the storage type
  1   dle_gemm                       the decoder: fp32 logits [rows, 32] over the weight padded to 32 rows
  1   dle_ctc_greedy_packed          log_softmax, argmax, the CTC collapse
All block outputs of a dense run stay alive until the run ends.  The BatchNorm coefficients stay fp32 (convnets.infer.fold_bn);
the 16-bit weights are unmodified.

Host synchronisation.  The lengths are known on the host, so every cu table is built there and uploaded in ONE copy; the only
device-to-host read of a batch is the one that brings the tokens (or the log-probabilities) back.  `d2h_reads` counts them.

Not built (one-line errors): fp32, what model.check_config rejects, utterances of fewer than 2 frames (the reference's
normalisation gives NaN there).  No CPU path.
"""
import numpy as np
import torch

from .. import _cabi as C
from .. import functional as F
from ..convnets.infer import fold_bn
from ..quartznet.features import FilterbankFeatures
from .model import BN_EPS, JasperModel, convert_v1_state_dict, load_config, normalize_keys


class _Unit:
    __slots__ = ("w", "scale", "shift", "stride", "dilation")


class _Block:
    __slots__ = ("units", "panes", "dense")


class JasperRecognizer:
    def __init__(self, model_or_state_dict, config=None, dtype=torch.float16, device=None, pad_leading=16):
        """model_or_state_dict: a JasperModel (left untouched) or the reference's state dict (then `config` is the reference's
        YAML, a path or the dict it holds).  dtype: torch.float16 or torch.bfloat16.  pad_leading: zero frames in front of every
        utterance's normalised features (inference.py --pad_leading)."""
        if dtype == torch.float32:
            raise ValueError("this path computes in 16 bits: pass torch.float16 or torch.bfloat16 (the reference's fp32 / TF32 "
                             "recipes are not built)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("dtype must be torch.float16 or torch.bfloat16 (got %s)" % (dtype,))
        if int(pad_leading) < 0:
            raise ValueError("pad_leading must not be negative (got %r)" % (pad_leading,))
        if isinstance(model_or_state_dict, JasperModel):
            model = model_or_state_dict
        else:
            if config is None:
                raise ValueError("a state dict needs the model's YAML configuration")
            model = JasperModel(config).load_state_dict(model_or_state_dict)
        self.cfg, self.labels = model.cfg, list(model.labels)
        self.n_classes = len(self.labels) + 1
        if self.n_classes > 32:
            raise ValueError("%d classes: the decoder is padded to 32 rows" % self.n_classes)
        self.dev = dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise C.DleError("JasperRecognizer runs on the MI355X only (got device %s); there is no CPU path" % dev)
        self.dtype = dtype
        self.pad_leading = int(pad_leading)
        self.features = FilterbankFeatures(**model.features)
        self.n_feat = model.blocks[0]["infilters"]
        P = model.params

        def bn(p):
            s, h = fold_bn(P[p + "weight"], P[p + "bias"], P[p + "running_mean"], P[p + "running_var"], BN_EPS)
            return s.to(dev), h.to(dev)

        self.blocks = []
        with torch.no_grad():
            for n, b in enumerate(model.blocks):
                pre = "encoder.layers.%d." % n
                blk = _Block()
                blk.units, blk.panes, blk.dense = [], [], b["dense"]
                for r in range(b["repeat"]):
                    u = _Unit()
                    u.stride, u.dilation = b["stride"], b["dilation"]
                    u.w = F.pack_conv1d_weight(P["%sconv.%d.weight" % (pre, 4 * r)].float(), dtype).to(dev)
                    u.scale, u.shift = bn("%sconv.%d." % (pre, 4 * r + 1))
                    blk.units.append(u)
                for j in range(len(b["panes"])):
                    w = P["%sres.%d.0.weight" % (pre, j)].float()[:, :, 0]
                    blk.panes.append((w.to(dtype).contiguous().reshape(w.shape[0], 1, 1, w.shape[1]).to(dev),) +
                                     bn("%sres.%d.1." % (pre, j)))
                self.blocks.append(blk)
            self.dec_w, self.dec_b = F.pad_ctc_decoder(P["decoder.layers.0.weight"].float(), P["decoder.layers.0.bias"], dtype, 32)
            self.dec_w, self.dec_b = self.dec_w.to(dev), self.dec_b.to(dev)
        self.d2h_reads = 0          # device-to-host copies so far: one per batch

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, config_path, ema=False, **kw):
        """The reference's checkpoint file, or what it holds: {'state_dict', 'ema_state_dict', ...} (inference.py:276-281 reads
        'ema_state_dict' under --ema), or a bare state dict; the key names of the first release are converted
        (convert_v1_state_dict)."""
        ckpt = path_or_ckpt
        if not isinstance(ckpt, dict):
            if str(ckpt).endswith(".nemo"):
                raise ValueError(".nemo checkpoints are not built: convert to a torch checkpoint with the reference's tools")
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        if "state_dict" in ckpt or "ema_state_dict" in ckpt:
            key = "ema_state_dict" if (ema and ckpt.get("ema_state_dict") is not None) else "state_dict"
            if ckpt.get(key) is None:
                raise KeyError("not a Jasper checkpoint: no %r entry" % key)
            state = ckpt[key]
        else:
            state = ckpt
        return cls(convert_v1_state_dict(normalize_keys(state)), config=load_config(config_path), **kw)

    # ------------------------------------------------------------------ the forward pass
    def _tables(self, lens):
        """Every cu table of the chain on the host, one upload: the padded input lengths, and one more table behind each strided
        sub-block."""
        cur = [n + self.pad_leading for n in lens]
        tabs = [cur]
        for blk in self.blocks:
            for u in blk.units:
                if u.stride != 1:
                    cur = [(n - 1) // u.stride + 1 for n in cur]
                    tabs.append(cur)
        host = np.stack([np.concatenate([[0], np.cumsum(t)]) for t in tabs]).astype(np.int32)
        return tabs, torch.from_numpy(host).to(self.dev)

    def _forward(self, feats, lens, want_logp):
        dev, dt = self.dev, self.dtype
        if len(feats) != len(lens) or not feats:
            raise ValueError("features and lens must be non-empty lists of one length")
        lens = [int(n) for n in lens]
        for i, (f, n) in enumerate(zip(feats, lens)):
            if f.dim() != 2 or f.shape[0] != self.n_feat or f.shape[1] < n:
                raise ValueError("utterance %d: features must be [%d, >= %d frames] (got %s)" % (i, self.n_feat, n, tuple(f.shape)))
            if n < 2:
                raise ValueError("utterance %d has %d frame(s): fewer than 2 frames are not built (the reference's per-feature "
                                 "standard deviation is NaN there)" % (i, n))
        b, t_pad = len(lens), max(lens)
        with torch.no_grad():
            x = torch.zeros((b, self.n_feat, t_pad), dtype=torch.float32)
            for i, (f, n) in enumerate(zip(feats, lens)):
                x[i, :, :n] = f[:, :n].to(torch.float32)
            x = x.to(dev)
            tabs, cu_all = self._tables(lens)
            ti, cu, total = 0, cu_all[0], sum(tabs[0])
            h = F.qn_normalize_pack_lead(x, cu, total, dt, self.pad_leading)
            xs = [h]                                                           # the encoder's list (model.py:204-209)
            for blk in self.blocks:
                res = None
                for (w, s, sh), src in zip(blk.panes, xs):
                    res = F.conv2d_fwd_affine(src.view(1, 1, total, src.shape[1]), w, s, sh,
                                              residual=None if res is None else res.view(1, 1, total, -1),
                                              relu=False).view(total, w.shape[0])
                h, last = xs[-1], len(blk.units) - 1
                for i, u in enumerate(blk.units):
                    r = res if i == last else None
                    if u.stride != 1:
                        ti += 1
                        cu_o, total_o = cu_all[ti], sum(tabs[ti])
                        h = F.conv1d_bn_packed_fwd(h, u.w, u.scale, u.shift, cu, cu_o, total_o, stride=u.stride,
                                                   dilation=u.dilation, residual=r, relu=True)
                        cu, total = cu_o, total_o
                    else:
                        h = F.conv1d_bn_packed_fwd(h, u.w, u.scale, u.shift, cu, stride=1, dilation=u.dilation, residual=r,
                                                   relu=True)
                xs = xs + [h] if blk.dense else [h]
            h = xs[-1]
            logits = F.gemm(h, self.dec_w, total, 32, h.shape[1], True, True, out_dtype=torch.float32, bias=self.dec_b)
            logp, ids, tokens, n_tokens = F.ctc_greedy_packed(logits, cu, self.n_classes, want_logp=want_logp)
        return tabs[ti], cu, logp, ids, tokens, n_tokens

    def log_probs(self, features, lens):
        """features: a list of fp32 log-mel [n_feat, >= len_b] (what FilterbankFeatures returns), lens: the frame counts
        -> a list of fp32 [out_len_b, n_classes] log-probabilities (device tensors)."""
        out_lens, cu, logp, _, _, _ = self._forward(features, lens, True)
        return list(torch.split(logp, out_lens))

    def decode(self, features, lens, want_logp=False):
        """-> (list of strings, list of int32 id tensors per utterance (host), list of log-probabilities or None)."""
        out_lens, cu, logp, ids, tokens, n_tokens = self._forward(features, lens, want_logp)
        host = torch.cat([n_tokens, ids, tokens]).cpu()                       # the batch's one device-to-host read
        self.d2h_reads += 1
        b, total = len(out_lens), sum(out_lens)
        n_tok, ids_h, tok_h = host[:b].tolist(), host[b:b + total], host[b + total:]
        texts, frames, start = [], [], 0
        for i, n in enumerate(out_lens):
            texts.append("".join(self.labels[c] for c in tok_h[start:start + n_tok[i]].tolist()))
            frames.append(ids_h[start:start + n])
            start += n
        return texts, frames, (list(torch.split(logp, out_lens)) if logp is not None else None)

    def transcribe(self, waves, generator=None):
        """a list of fp32 waveforms (16 kHz, [-1, 1]) -> a list of strings."""
        feats, lens = self.features(waves, generator)
        return self.decode(feats, lens)[0]
