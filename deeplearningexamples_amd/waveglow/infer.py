"""WaveGlow inference on the gfx950 library: mel spectrogram -> audio, the reverse flow of WaveGlow.infer
(SpeechSynthesis/Tacotron2/waveglow/model.py:234-272) and the bias removal of waveglow/denoiser.py.

The same GEMM formulation as the train step (waveglow/engine.py), run backwards through the flows and keeping nothing:
  * upsampling: ONE GEMM over `frames` row blocks; its output [B, frames*256, 80] read as [M, 640] is the grouped spectrogram of
    exactly the frames*256 samples the reference keeps after its `time_cutoff` trim (kernel - stride = 768 samples);
  * per flow k = n_flows-1 .. 0:  start GEMM (a0 [M, 8] -> [M, nc]);  the flow's cond layers as one GEMM [M, 640] -> [M, n_layers*2nc];
    per layer: dle_wg_taps, in GEMM (+ cond slice in the epilogue), dle_wg_gate_fwd, res_skip GEMM (+ the running halves);
    end GEMM (fp32 [M, 8] = b | log_s | 0);  dle_wg_flow_inv: affine coupling inverse, W^-1, the early-output noise and the
    16-bit `start` operand of the next flow, one launch.
The fp32 flow state [M, 8] is updated in place; after flow 0 it IS the audio [B, T].  One set of work buffers per (B, frames)
serves every flow and every call, so memory does not grow with n_flows (weights apart).  No CPU path.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from . import ops
from .model import UPSAMPLE_KERNEL, UPSAMPLE_STRIDE, WaveGlow, flow_channels


class WaveGlowVocoder:
    def __init__(self, model: WaveGlow, compute_dtype=torch.float16):
        self.model, self.cfg = model, model.cfg
        self.dev = dev = model.store.flat.device
        self.dtype = dt = compute_dtype
        wn = self.cfg["WN_config"]
        self.nc, self.nl, self.ks = nc, nl, ks = wn["n_channels"], wn["n_layers"], wn["kernel_size"]
        self.mel, self.ng, self.nf = self.cfg["n_mel_channels"], self.cfg["n_group"], self.cfg["n_flows"]
        if nc % 8 or self.mel % 8 or ks % 2 == 0:
            raise ValueError("n_channels and n_mel_channels must be multiples of 8, kernel_size odd")
        self.chans = flow_channels(self.cfg)
        self.n_rem = self.chans[-1][0]                                   # channels of the initial noise (model.py:187)
        self.early = [self.cfg["n_early_size"] if (k % self.cfg["n_early_every"] == 0 and k > 0) else 0 for k in range(self.nf)]
        # column of the noise rows each early output reads: the reference's z holds them after the initial channels, in the
        # order the reverse loop consumes them (infer_onnx, model.py:293-311)
        self.z_col, col = [0] * self.nf, self.n_rem
        for k in range(self.nf - 1, -1, -1):
            if self.early[k]:
                self.z_col[k] = col
                col += self.early[k]
        self.p = p = model.store
        kc = self.mel * self.ng
        cols = nl * 2 * nc                                               # cond / pre-activation columns of ONE flow
        self.w_cond = torch.zeros((self.nf * cols, kc), dtype=dt, device=dev)
        self.w_in = torch.zeros((self.nf * nl, 2 * nc, ks * nc), dtype=dt, device=dev)
        # res_skip operands: rows [0, nc) = residual half, [nc, 2nc) = skip half; the last layer has the skip half only
        self.w_rs = torch.zeros((self.nf, nl, 2 * nc, nc), dtype=dt, device=dev)
        self.w_start = torch.zeros((self.nf, nc, 8), dtype=dt, device=dev)
        self.w_end = torch.zeros((self.nf, 8, nc), dtype=dt, device=dev)  # rows >= 2 n_half stay zero
        entries, ld = [], []
        for k, (c, nh) in enumerate(self.chans):
            pre = "WN.%d." % k

            def normed(name, w16, cip=None, as_shape=None):
                v = p[name + ".weight_v"]
                entries.append(dict(v=v if as_shape is None else v.view(as_shape), g=p[name + ".weight_g"], w16=w16, cip=cip))
            normed(pre + "start", self.w_start[k], cip=8)
            entries.append(dict(v=p[pre + "end.weight"], g=None, w16=self.w_end[k]))
            for i in range(nl):
                z = k * nl + i
                normed(pre + "in_layers.%d" % i, self.w_in[z])
                # time-major spectrogram rows are (g, mel): the [2nc, 640, 1] weight read as [2nc, 80, 8] lands in that order
                normed(pre + "cond_layers.%d" % i, self.w_cond[z * 2 * nc:(z + 1) * 2 * nc], as_shape=(2 * nc, self.mel, self.ng))
                normed(pre + "res_skip_layers.%d" % i, self.w_rs[k, i] if i < nl - 1 else self.w_rs[k, i, nc:])
            ld.append((p.offsets["convinv.%d.conv.weight" % k][0], c))
        self.wn_table = ops.WeightNormTable(entries, dev)
        self.ld_table = ops.LogdetTable(ld, dev)
        self.logdets = torch.zeros(self.nf, dtype=torch.float32, device=dev)
        self.signs = torch.ones(self.nf, dtype=torch.float32, device=dev)
        self.winv_t = torch.zeros((self.nf, 64), dtype=torch.float32, device=dev)
        self._buffers = {}
        self.refresh()

    def refresh(self):
        """fp32 parameters -> 16-bit GEMM operands and every W^-T: at construction, and again after the model's weights change."""
        p = self.p
        self.w_up, self.b_up = ops.upsample_weight(p["upsample.weight"], p["upsample.bias"], self.dtype, UPSAMPLE_STRIDE)
        ops.weight_norm_fwd_batched(self.wn_table, self.dtype)
        ops.logdet_inv_batched(p.flat, self.ld_table, self.logdets, self.winv_t, self.signs)

    def _work(self, b, frames):
        """The work buffers of one (batch, frames) shape: shared by all flows, kept between calls."""
        key = (b, frames)
        w = self._buffers.get(key)
        if w is None:
            nc, nl, dt, dev = self.nc, self.nl, self.dtype, self.dev
            m = b * frames * UPSAMPLE_STRIDE // self.ng
            ntap = UPSAMPLE_KERNEL // UPSAMPLE_STRIDE

            def e(shape, dtype=dt):
                return torch.empty(shape, dtype=dtype, device=dev)
            w = dict(mel_cl=e((b * frames, self.mel)), col_mel=e((b * frames, ntap * self.mel)),
                     spect=e((b * frames, UPSAMPLE_STRIDE * self.mel)), cond=e((m, nl * 2 * nc)), s=e((m, nl * 2 * nc)),
                     xo=[e((m, 2 * nc)), e((m, 2 * nc))], col=e((m, self.ks * nc)), acts=e((m, nc)), a0=e((m, 8)),
                     o=e((m, 8), torch.float32), state=e((m, 8), torch.float32), noise=e((m, 8), torch.float32))
            self._buffers[key] = w
        return w

    def infer(self, mel, sigma=1.0, z=None):
        """mel fp32 [B, 80, frames] -> audio fp32 [B, frames*256].  z: the noise, [B, 8, frames*32] fp32 as infer_onnx takes it
        (the first n_remaining_channels channels start the flow, the others are the early outputs in the order they are used);
        None: drawn on the device.  The result is this vocoder's state buffer for the shape: the next call at the same shape
        overwrites it (clone() to keep it)."""
        C.require_cuda(mel, z)
        if mel.dim() != 3 or mel.shape[1] != self.mel or mel.dtype != torch.float32 or mel.shape[2] < 1:
            raise ValueError("mel must be fp32 [B, %d, frames]" % self.mel)
        nc, nl, ks, ng = self.nc, self.nl, self.ks, self.ng
        b, frames = mel.shape[0], mel.shape[2]
        t = frames * UPSAMPLE_STRIDE
        tg = t // ng
        m = b * tg
        w = self._work(b, frames)
        noise = w["noise"]
        if z is None:
            noise.normal_()
        else:
            if z.shape != (b, ng, tg) or z.dtype != torch.float32:
                raise ValueError("z must be fp32 [B, %d, frames*%d]" % (ng, UPSAMPLE_STRIDE // ng))
            noise.view(b, tg, ng).copy_(z.permute(0, 2, 1))              # row (b, t) = the 8 channels of z[b, :, t]
        # upsampling: channels-last 16-bit mel, its 4 frame taps, one GEMM -> the grouped spectrogram [M, 640]
        ntap = UPSAMPLE_KERNEL // UPSAMPLE_STRIDE
        ops.mel_rows(mel.contiguous(), w["mel_cl"])
        ops.taps(w["mel_cl"], b, frames, ntap, -1, 0, out=w["col_mel"])
        F.gemm(w["col_mel"], self.w_up, b * frames, UPSAMPLE_STRIDE * self.mel, ntap * self.mel, True, True, bias=self.b_up,
               out=w["spect"])
        spect = w["spect"].view(m, self.mel * ng)
        state, a0, o, xo, cond, s_all, col, acts = (w[k] for k in ("state", "a0", "o", "xo", "cond", "s", "col", "acts"))
        cols = nl * 2 * nc
        p = self.p
        ops.flow_inv_first(noise, self.n_rem, sigma, state, a0)
        for k in range(self.nf - 1, -1, -1):
            c, _ = self.chans[k]
            pre = "WN.%d." % k
            F.gemm(a0, self.w_start[k], m, nc, 8, True, True, bias=p[pre + "start.bias"], out=xo[0][:, :nc])
            xo[0][:, nc:].zero_()
            off = p.offsets[pre + "cond_layers.0.bias"][0]               # the flow's cond biases are contiguous, layer-major
            F.gemm(spect, self.w_cond[k * cols:(k + 1) * cols], m, cols, self.mel * ng, True, True, bias=p.flat[off:off + cols],
                   out=cond)
            cur = 0
            for i in range(nl):
                c0 = i * 2 * nc
                ops.taps(xo[cur][:, :nc], b, tg, ks, 2 ** i, ks // 2, out=col)
                s_i = s_all[:, c0:c0 + 2 * nc]
                F.gemm(col, self.w_in[k * nl + i], m, 2 * nc, ks * nc, True, True, out=s_i, bias=p[pre + "in_layers.%d.bias" % i],
                       act=C.ACT_ADD, mask_src=cond[:, c0:c0 + 2 * nc])
                ops.gate_fwd(s_i, nc, out=acts)
                b_rs = p[pre + "res_skip_layers.%d.bias" % i]
                if i < nl - 1:
                    F.gemm(acts, self.w_rs[k, i], m, 2 * nc, nc, True, True, bias=b_rs, act=C.ACT_ADD, mask_src=xo[cur],
                           out=xo[1 - cur])
                else:                                                    # the last layer has the skip half only
                    F.gemm(acts, self.w_rs[k, i, nc:], m, nc, nc, True, True, bias=b_rs, act=C.ACT_ADD, mask_src=xo[cur][:, nc:],
                           out=xo[1 - cur][:, nc:])
                cur = 1 - cur
            F.gemm(xo[cur][:, nc:], self.w_end[k], m, 8, nc, True, True, bias=p.slot(pre + "end.bias"), out=o)
            nxt = self.chans[k - 1][0] if k > 0 else 0
            ops.flow_inv(state, o, self.winv_t[k], c, out=state, a0=a0 if k > 0 else None, next_c=nxt, early=self.early[k],
                         noise=noise, z_col=self.z_col[k], sigma=sigma)
        return state.view(b, t)


class STFT:
    """The short-time Fourier transform pair of tacotron2_common/stft.py: a strided convolution with the windowed Fourier basis
    and a strided transposed convolution with its windowed pseudo-inverse, then the window-envelope correction.  Both
    convolutions are written as what they are -- frames x basis products, and an overlap-add -- in plain torch: this runs once
    per utterance."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, device="cpu"):
        if win_length > filter_length:
            raise ValueError("win_length must not exceed filter_length")
        self.n, self.hop, self.win = filter_length, hop_length, win_length
        n, half = filter_length, filter_length // 2 + 1
        spec = torch.fft.fft(torch.eye(n, dtype=torch.float64))[:half]
        basis = torch.cat([spec.real, spec.imag], 0)                     # [2 * half, n]
        inv = torch.linalg.pinv((n / hop_length) * basis).t().to(torch.float32)
        window = torch.zeros(n, dtype=torch.float64)
        lo = (n - win_length) // 2
        window[lo:lo + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
        wf = window.to(torch.float32)
        self.window_sq = (window * window).to(torch.float32).to(device)
        self.forward_basis = (basis.to(torch.float32) * wf).to(device)   # [2 * half, n]
        self.inverse_basis = (inv * wf).to(device)                       # [2 * half, n]

    def _overlap_add(self, cols):
        """cols [B, n, frames]: frame f added at sample f * hop -> [B, 1, n + hop * (frames - 1)]."""
        frames = cols.shape[-1]
        length = self.n + self.hop * (frames - 1)
        return torch.nn.functional.fold(cols, (1, length), (1, self.n), stride=(1, self.hop))[:, :, 0]

    def transform(self, x):
        """x [B, T] -> (magnitude, phase), each [B, n/2 + 1, T / hop + 1]."""
        pad = self.n // 2
        padded = torch.nn.functional.pad(x[:, None, :], (pad, pad), mode="reflect")[:, 0]
        y = (padded.unfold(1, self.n, self.hop) @ self.forward_basis.t()).transpose(1, 2)
        half = self.n // 2 + 1
        re, im = y[:, :half], y[:, half:]
        return torch.sqrt(re * re + im * im), torch.atan2(im, re)

    def inverse(self, magnitude, phase):
        """-> [B, 1, (frames - 1) * hop]."""
        spec = torch.cat([magnitude * torch.cos(phase), magnitude * torch.sin(phase)], 1)
        y = self._overlap_add(self.inverse_basis.t() @ spec)
        frames = magnitude.shape[-1]
        env = self._overlap_add(self.window_sq[None, :, None].expand(1, self.n, frames).contiguous())[0, 0]
        ok = env > torch.finfo(torch.float32).tiny                       # the sum of the squared windows over the frames
        y = torch.where(ok, y / torch.where(ok, env, torch.ones_like(env)), y) * (float(self.n) / self.hop)
        return y[:, :, self.n // 2:-(self.n // 2)]


class Denoiser:
    """waveglow/denoiser.py: the magnitude spectrum of what the vocoder emits for an empty spectrogram (sigma = 0), scaled by
    `strength`, is subtracted from the audio's magnitudes.  `vocoder`: anything with infer(mel, sigma=...) -> audio [1, T]."""

    def __init__(self, vocoder, filter_length=1024, n_overlap=4, win_length=1024, mode="zeros", device=None, n_mel_channels=80):
        device = device if device is not None else getattr(vocoder, "dev", "cpu")
        self.stft = STFT(filter_length, filter_length // n_overlap, win_length, device)
        if mode == "zeros":
            mel = torch.zeros((1, n_mel_channels, 88), dtype=torch.float32, device=device)
        elif mode == "normal":
            mel = torch.randn((1, n_mel_channels, 88), dtype=torch.float32, device=device)
        else:
            raise ValueError("Mode %s is not supported" % mode)
        bias_audio = vocoder.infer(mel, sigma=0.0).float()
        bias_spec, _ = self.stft.transform(bias_audio)
        self.bias_spec = bias_spec[:, :, :1].clone()

    def forward(self, audio, strength=0.1):
        """audio fp32 [B, T] -> [B, 1, T]."""
        spec, angles = self.stft.transform(audio)
        return self.stft.inverse(torch.clamp(spec - self.bias_spec * strength, min=0.0), angles)

    __call__ = forward
