"""HiFi-GAN inference on the gfx950 library: mel spectrogram -> audio, Generator.forward of
SpeechSynthesis/HiFiGAN/hifigan/models.py:208-222 after remove_weight_norm, and the bias removal of models.py:235-270.

Activations are channels-last [B, T, C] in 16 bits; every convolution is ONE launch of dle_conv1d_lrelu_fwd
(csrc/hifigan.hip) that also carries the leaky ReLU in front of it and the elementwise steps behind it:
  * mel [B, 80, T] -> [B, T, 80] 16-bit (one layout launch), conv_pre (no activation);
  * per stage: the ConvTranspose1d as a 3-tap convolution on the packed weight (functional.pack_upsample_weight) with the stage's
    leaky ReLU(0.1) on its input -- its [B, T, u C] output IS the [B, T u, C] tensor the blocks read; then the residual blocks,
    one after the other: a block's `xt + x` is add1 of the second convolution of each pair, the running `xs += block(x)` is add2
    of each block's last convolution (written in place over xs) and `xs / num_kernels` its alpha in the last block;
  * conv_post + leaky ReLU(0.01) + tanh: dle_hfg_post_fwd, fp32 audio.
For the V1 configuration 1 + 4 (1 + 3 x 6) = 77 convolution launches + the layout launch + the output kernel, one stream, one
chain, no allocation after the first call at a shape.  Eager calls keep the work buffers of the most recent (B, T) only (V1 at
16 x 800 frames holds about 3.3 GB of them), so a list of batches of many lengths does not grow memory; with graphs=True every
captured shape keeps its own.  Where the reference rounds xs after every block and once more after the
division, this path rounds the stage's output once per block (the sum so far) -- never more roundings than the reference.

Weights are folded (g v / ||v||) and packed once at construction.  No CPU path.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import GraphCache, gpu_device, require_16bit
from ..waveglow.infer import STFT
from ..waveglow.infer import Denoiser as _WaveGlowDenoiser
from .model import LRELU_SLOPE, N_MEL, HifiGanGenerator, check_config, normalize_keys

POST_SLOPE = 0.01            # the last F.leaky_relu(x) of Generator.forward takes torch's default slope (models.py:218)


class _Conv:
    __slots__ = ("w", "bias", "ksize", "dilation", "ko")

    def __init__(self, w, bias, dilation):
        self.w, self.bias, self.dilation = w, bias, dilation
        self.ko, self.ksize = w.shape[0], w.shape[1]


class HifiGanVocoder:
    def __init__(self, model_or_state, config=None, dtype=torch.float16, device=None, graphs=False):
        """model_or_state: a HifiGanGenerator (left untouched) or the reference's generator state dict (then `config` is
        required; any device; `module.` prefixes, the older flat resblock keys and folded `weight` tensors allowed).
        dtype: torch.float16 or torch.bfloat16.  graphs: replay one captured graph per (B, T)."""
        require_16bit(dtype, "HifiGanVocoder")
        if isinstance(model_or_state, HifiGanGenerator):
            model = model_or_state
        else:
            if config is None:
                raise ValueError("a state dict needs its config (upsample_rates, ..., resblock_dilation_sizes)")
            model = HifiGanGenerator(config, device="cpu").load_state_dict(model_or_state)
        self.cfg = cfg = check_config(model.cfg)
        self.dev = dev = gpu_device(device, "HifiGanVocoder")
        self.dtype = dtype
        self.rates = list(cfg["upsample_rates"])
        self.hop = 1
        for u in self.rates:
            self.hop *= u
        self.num_kernels = len(cfg["resblock_kernel_sizes"])
        by_name = {l.name: l for l in model.layers}

        def conv(name):
            l = by_name[name]
            w = model.folded_weight(name)
            if l.kind == "up":
                w16 = F.pack_upsample_weight(w, l.stride, dtype)
                bias = model.params[name + ".bias"].float().repeat(l.stride)
            else:
                w16 = F.pack_conv1d_weight(w, dtype)
                bias = model.params[name + ".bias"].float()
            return _Conv(w16.to(dev), bias.contiguous().to(dev), l.dilation)
        with torch.no_grad():
            self.pre = conv("conv_pre")
            self.ups = [conv("ups.%d" % i) for i in range(len(self.rates))]
            self.blocks = []                  # [stage][block] -> [(first conv, second conv or None)]
            for i in range(len(self.rates)):
                stage = []
                for j in range(self.num_kernels):
                    p = "resblocks.%d.%d." % (i, j)
                    if cfg["resblock"] == "1":
                        stage.append([(conv(p + "convs1.%d" % n), conv(p + "convs2.%d" % n)) for n in range(3)])
                    else:
                        stage.append([(conv(p + "convs.%d" % n), None) for n in range(2)])
                self.blocks.append(stage)
            post = by_name["conv_post"]
            self.post_w = model.folded_weight("conv_post")[0].t().to(dtype).contiguous().to(dev)      # [ksize, C]
            self.post_bias = model.params["conv_post.bias"].float().contiguous().to(dev)
            self.post_c = post.cin
        self._buffers = {}
        self._graphs = GraphCache(graphs)     # (B, T) -> GraphedStep

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, ema=False, config=None, **kw):
        """The reference's checkpoint file (or the dict it holds): {'generator': sd, 'gen_ema': sd or None, 'config': {...},
        'train_setup': {...}}.  ema: take the averaged weights (models.py load_and_setup_model)."""
        ckpt = path_or_ckpt
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        if "generator" not in ckpt:
            raise KeyError("not a HiFi-GAN checkpoint: no 'generator' entry")
        state = ckpt["generator"]
        if ema:
            if ckpt.get("gen_ema") is None:
                raise KeyError("the checkpoint holds no EMA weights ('gen_ema')")
            state = ckpt["gen_ema"]
        config = config if config is not None else ckpt.get("config")
        if config is None:
            raise KeyError("the checkpoint holds no 'config': pass config=")
        return cls(normalize_keys(state), config=config, **kw)

    def _work(self, b, t):
        key = (b, t)
        w = self._buffers.get(key)
        if w is None:
            if not self._graphs.graphs:       # eager: the buffers of ONE shape, the most recent (a captured graph owns its shape's)
                self._buffers.clear()
            def e(*shape, dtype=self.dtype):
                return torch.empty(shape, dtype=dtype, device=self.dev)
            w = dict(mel_cl=e(b * t, N_MEL), h=e(b, t, self.pre.ko), stages=[], audio=e(b, t * self.hop, dtype=torch.float32))
            tt = t
            for i, u in enumerate(self.rates):
                ch = self.ups[i].ko // u
                # u: the upsampled tensor [B, T, u ch] = [B, T u, ch]; xt / xa: a block's temporaries; xs: the sum over the blocks
                w["stages"].append(dict(u=e(b, tt, u * ch), xt=e(b, tt * u, ch), xa=e(b, tt * u, ch), xb=e(b, tt * u, ch),
                                        xs=e(b, tt * u, ch)))
                tt *= u
            self._buffers[key] = w
        return w

    def _forward(self, mel):
        b, _, t = mel.shape
        w = self._work(b, t)
        C.call("dle_nchw_to_nhwc", C.ptr(mel), C.ptr(w["mel_cl"]), b, N_MEL, t, N_MEL, C.dt(self.dtype), C.stream())
        h = F.conv1d_lrelu_fwd(w["mel_cl"].view(b, t, N_MEL), self.pre.w, self.pre.bias, out=w["h"])
        nk = self.num_kernels
        for i, u in enumerate(self.rates):
            s = w["stages"][i]
            up = self.ups[i]
            F.conv1d_lrelu_fwd(h, up.w, up.bias, slope=LRELU_SLOPE, out=s["u"])
            x0 = s["u"].view(b, h.shape[1] * u, up.ko // u)
            for j, block in enumerate(self.blocks[i]):
                x = x0
                for n, (c1, c2) in enumerate(block):
                    last = n == len(block) - 1
                    # where this pair's `xt + x` goes: the running sum for the block's last pair, else a buffer that is not x
                    if last:
                        out, add2, alpha = s["xs"], (s["xs"] if j else None), (1.0 / nk if j == nk - 1 else 1.0)
                    else:
                        out, add2, alpha = (s["xb"] if x is s["xa"] else s["xa"]), None, 1.0
                    if c2 is not None:
                        xt = F.conv1d_lrelu_fwd(x, c1.w, c1.bias, dilation=c1.dilation, slope=LRELU_SLOPE, out=s["xt"])
                        x = F.conv1d_lrelu_fwd(xt, c2.w, c2.bias, dilation=c2.dilation, slope=LRELU_SLOPE, alpha=alpha, add1=x,
                                               add2=add2, out=out)
                    else:
                        x = F.conv1d_lrelu_fwd(x, c1.w, c1.bias, dilation=c1.dilation, slope=LRELU_SLOPE, alpha=alpha, add1=x,
                                               add2=add2, out=out)
            h = s["xs"]
        return F.hfg_post_fwd(h, self.post_w, self.post_bias, slope=POST_SLOPE, out=w["audio"])

    def infer(self, mel, sigma=None):
        """mel [B, 80, T] fp32 or 16-bit -> audio fp32 [B, T * prod(upsample_rates)].  The result is a buffer this vocoder owns
        for the shape: the next call at the same shape overwrites it (clone() to keep it).  `sigma` is accepted and ignored (the
        calling convention of the project's vocoders; this network draws no noise)."""
        C.require_cuda(mel)
        if mel.dim() != 3 or mel.shape[1] != N_MEL or mel.shape[2] < 1 or mel.dtype not in (torch.float32, torch.float16,
                                                                                            torch.bfloat16):
            raise ValueError("mel must be [B, %d, T] in fp32, fp16 or bf16" % N_MEL)
        b, t = mel.shape[0], mel.shape[2]
        if b == 0:
            return torch.empty((0, t * self.hop), dtype=torch.float32, device=self.dev)
        mel = mel.float().contiguous()                                   # (a 16-bit spectrogram widens exactly)
        with torch.no_grad():
            return self._graphs.run((b, t), self._forward, mel)

    __call__ = infer


class Denoiser(_WaveGlowDenoiser):
    """hifigan/models.py:235-270: as the WaveGlow denoiser, the bias audio being what the generator emits for a zero (or normal)
    spectrogram of 88 frames -- no sigma."""

    def __init__(self, vocoder, filter_length=1024, n_overlap=4, win_length=1024, mode="zeros", device=None):
        device = device if device is not None else vocoder.dev
        self.stft = STFT(filter_length, filter_length // n_overlap, win_length, device)
        if mode == "zeros":
            mel = torch.zeros((1, N_MEL, 88), dtype=torch.float32, device=device)
        elif mode == "normal":
            mel = torch.randn((1, N_MEL, 88), dtype=torch.float32, device=device)
        else:
            raise ValueError("Mode %s is not supported" % mode)
        bias_spec, _ = self.stft.transform(vocoder.infer(mel).float())
        self.bias_spec = bias_spec[:, :, :1].clone()
