"""QuartzNet inference on the gfx950 library: log-mel features -> log-probabilities / transcripts, the forward of
SpeechRecognition/QuartzNet/quartznet/model.py:352-364 (QuartzNet.forward with use_conv_masks) behind the front end of
common/features.py:200-302 and in front of GreedyCTCDecoder and common/helpers.py:35-61, as inference.py:330-375 chains them.

Layout.  Activations are 16-bit, channels-last and PACKED: [total_rows, C] with device int32 cu tables; there are no padding rows.
The reference zeroes the frames behind an utterance's length in front of every convolution, so its result for an utterance does
not depend on what shares the batch; neither does it here.

Launches, for a configuration of U separable units, R residual blocks and a last unit that is not separable (15x5: 77, 15, 1):
  1      dle_qn_normalize_pack            per-feature normalisation, mask, transpose, 16-bit cast
  U      dle_tcs_conv1d_packed_fwd        depthwise + pointwise + BatchNorm (+ residual) + ReLU, one launch per unit
  R + 1  dle_conv2d_fwd_affine            the residual branch of a block (1x1 conv + BatchNorm, computed FIRST and consumed by the
                                          block's last unit) and Conv3, as 1x1 convolutions over [1, 1, rows, C]
  1      dle_gemm                         the decoder: fp32 logits [rows, 32] over the weight padded to 32 rows
  1      dle_ctc_greedy_packed            log_softmax, argmax, the CTC collapse
The BatchNorm coefficients stay fp32 (utils.state.fold_bn); the 16-bit weights are unmodified.

Host synchronisation.  The lengths are known on the host, so every cu table is built there and uploaded in ONE copy; the only
device-to-host read of a batch is the one that brings the tokens (or the log-probabilities) back.  `d2h_reads` counts them.

Not built (one-line errors): fp32, a unit that is not separable with ksize != 1, what model.check_config rejects, utterances of
fewer than 2 frames (the reference's normalisation gives NaN there).  No CPU path.

CTCRecognizer holds what this recognizer shares with Jasper's (jasper/infer.py): everything but the weight packing of a block and
the block loop.
"""
import numpy as np
import torch

from .. import functional as F
from ..utils.frontend import gpu_device, require_16bit
from ..utils.state import fold_bn, load_config
from .features import FilterbankFeatures
from .model import BN_EPS, QuartzNetModel


class _Unit:
    __slots__ = ("dw", "pw", "scale", "shift", "ksize", "stride", "dilation", "separable")


class _Block:
    __slots__ = ("units", "res")


class CTCRecognizer:
    """Features -> packed encoder rows -> decoder GEMM -> greedy CTC.  A subclass names its host model class (MODEL), packs one
    block's weights (_pack_block; every unit it returns has a `stride`) and runs the encoder (_encode)."""
    MODEL = None

    def __init__(self, model_or_state_dict, config=None, dtype=torch.float16, device=None):
        """model_or_state_dict: a MODEL (left untouched) or the reference's state dict (then `config` is the reference's
        YAML, a path or the dict it holds).  dtype: torch.float16 or torch.bfloat16."""
        who = type(self).__name__
        require_16bit(dtype, who)
        if isinstance(model_or_state_dict, self.MODEL):
            model = model_or_state_dict
        else:
            if config is None:
                raise ValueError("a state dict needs the model's YAML configuration")
            model = self.MODEL(config).load_state_dict(model_or_state_dict)
        self.cfg, self.labels = model.cfg, list(model.labels)
        self.n_classes = len(self.labels) + 1
        if self.n_classes > 32:
            raise ValueError("%d classes: the decoder is padded to 32 rows" % self.n_classes)
        self.dev = dev = gpu_device(device, who)
        self.dtype = dtype
        self.features = FilterbankFeatures(**model.features)
        self.n_feat = model.blocks[0]["infilters"]
        P = model.params

        def bn(p):
            s, h = fold_bn(P[p + "weight"], P[p + "bias"], P[p + "running_mean"], P[p + "running_var"], BN_EPS)
            return s.to(dev), h.to(dev)

        with torch.no_grad():
            self.blocks = [self._pack_block(n, b, P, bn) for n, b in enumerate(model.blocks)]
            self.dec_w, self.dec_b = F.pad_ctc_decoder(P["decoder.layers.0.weight"].float(), P["decoder.layers.0.bias"], dtype, 32)
            self.dec_w, self.dec_b = self.dec_w.to(dev), self.dec_b.to(dev)
        self.d2h_reads = 0          # device-to-host copies so far: one per batch

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, config_path, ema=False, **kw):
        """The reference's checkpoint file, or what it holds: {'state_dict', 'ema_state_dict', ...} (inference.py reads
        'ema_state_dict' under --ema when the checkpoint has one, 'state_dict' otherwise), or a bare state dict.  The keys are
        cleaned up by MODEL.normalize_keys when the state is loaded."""
        ckpt = path_or_ckpt
        if not isinstance(ckpt, dict):
            if str(ckpt).endswith(".nemo"):
                raise ValueError(".nemo checkpoints are not built: convert to a torch checkpoint with the reference's tools")
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        if "state_dict" in ckpt or "ema_state_dict" in ckpt:
            key = "ema_state_dict" if (ema and ckpt.get("ema_state_dict") is not None) else "state_dict"
            if ckpt.get(key) is None:
                raise KeyError("not a %s checkpoint: no %r entry" % (cls.MODEL.NAME, key))
            state = ckpt[key]
        else:
            state = ckpt
        return cls(state, config=load_config(config_path), **kw)

    # ------------------------------------------------------------------ the forward pass
    def _tables(self, lens, lead=0):
        """Every cu table of the chain on the host, one upload: the input lengths (each with `lead` rows in front), and one more
        table behind each strided unit."""
        cur = [n + lead for n in lens]
        tabs = [cur]
        for blk in self.blocks:
            for u in blk.units:
                if u.stride != 1:
                    cur = [(n - 1) // u.stride + 1 for n in cur]
                    tabs.append(cur)
        host = np.stack([np.concatenate([[0], np.cumsum(t)]) for t in tabs]).astype(np.int32)
        return tabs, torch.from_numpy(host).to(self.dev)

    def _forward(self, feats, lens, want_logp):
        if len(feats) != len(lens) or not feats:
            raise ValueError("features and lens must be non-empty lists of one length")
        lens = [int(n) for n in lens]
        for i, (f, n) in enumerate(zip(feats, lens)):
            if f.dim() != 2 or f.shape[0] != self.n_feat or f.shape[1] < n:
                raise ValueError("utterance %d: features must be [%d, >= %d frames] (got %s)" % (i, self.n_feat, n, tuple(f.shape)))
            if n < 2:
                raise ValueError("utterance %d has %d frame(s): fewer than 2 frames are not built (the reference's per-feature "
                                 "standard deviation is NaN there)" % (i, n))
        with torch.no_grad():
            x = torch.zeros((len(lens), self.n_feat, max(lens)), dtype=torch.float32)
            for i, (f, n) in enumerate(zip(feats, lens)):
                x[i, :, :n] = f[:, :n].to(torch.float32)
            h, out_lens, cu = self._encode(x.to(self.dev), lens)
            logits = F.gemm(h, self.dec_w, h.shape[0], 32, h.shape[1], True, True, out_dtype=torch.float32, bias=self.dec_b)
            logp, ids, tokens, n_tokens = F.ctc_greedy_packed(logits, cu, self.n_classes, want_logp=want_logp)
        return out_lens, cu, logp, ids, tokens, n_tokens

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


class QuartzNetRecognizer(CTCRecognizer):
    MODEL = QuartzNetModel

    def _pack_block(self, n, b, P, bn):
        dev, dtype = self.dev, self.dtype
        pre = "encoder.layers.%d." % n
        blk = _Block()
        blk.units, m = [], 0
        for r in range(b["repeat"]):
            u = _Unit()
            u.ksize, u.stride, u.dilation, u.separable = b["kernel_size"], b["stride"], b["dilation"], b["separable"]
            if b["separable"]:
                u.dw = F.pack_depthwise_weight(P["%smconv.%d.weight" % (pre, m)].float(), dtype).to(dev)
                u.pw = P["%smconv.%d.weight" % (pre, m + 1)].float()[:, :, 0].to(dtype).contiguous().to(dev)
                u.scale, u.shift = bn("%smconv.%d." % (pre, m + 2))
                m += 5
            else:
                if b["kernel_size"] != 1 or b["stride"] != 1:
                    raise ValueError("block %d: a unit that is not separable is built for kernel_size 1, stride 1 only" % n)
                u.dw = None
                w = P["%smconv.%d.weight" % (pre, m)].float()[:, :, 0]
                u.pw = w.to(dtype).contiguous().reshape(w.shape[0], 1, 1, w.shape[1]).to(dev)
                u.scale, u.shift = bn("%smconv.%d." % (pre, m + 1))
                m += 4
            blk.units.append(u)
        blk.res = None
        if b["residual"]:
            w = P[pre + "res.0.0.weight"].float()[:, :, 0]
            blk.res = (w.to(dtype).contiguous().reshape(w.shape[0], 1, 1, w.shape[1]).to(dev),) + bn(pre + "res.0.1.")
        return blk

    def _encode(self, x, lens):
        """x: fp32 [B, n_feat, max len] on the device -> (the packed encoder output, its row counts, its cu table)."""
        tabs, cu_all = self._tables(lens)
        ti, cu, total = 0, cu_all[0], sum(lens)
        h = F.qn_normalize_pack(x, cu, total, self.dtype)
        for blk in self.blocks:
            res = None
            if blk.res is not None:
                w, s, sh = blk.res
                res = F.conv2d_fwd_affine(h.view(1, 1, total, h.shape[1]), w, s, sh, relu=False).view(total, w.shape[0])
            last = len(blk.units) - 1
            for i, u in enumerate(blk.units):
                r = res if i == last else None
                if not u.separable:
                    h = F.conv2d_fwd_affine(h.view(1, 1, total, h.shape[1]), u.pw, u.scale, u.shift,
                                            residual=None if r is None else r.view(1, 1, total, -1), relu=True).view(total, -1)
                elif u.stride != 1:
                    ti += 1
                    cu_o, total_o = cu_all[ti], sum(tabs[ti])
                    h = F.tcs_conv1d_packed_fwd(h, u.dw, u.pw, u.scale, u.shift, cu, cu_o, total_o, stride=u.stride,
                                                dilation=u.dilation, residual=r, relu=True)
                    cu, total = cu_o, total_o
                else:
                    h = F.tcs_conv1d_packed_fwd(h, u.dw, u.pw, u.scale, u.shift, cu, stride=1, dilation=u.dilation, residual=r,
                                                relu=True)
        return h, tabs[ti], cu
