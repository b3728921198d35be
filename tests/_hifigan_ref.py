"""float64 reference of the HiFi-GAN generator and the seeded weights of its tests (tests/ and tools/ only).

forward64: Generator.forward (hifigan/models.py:208-222) on the CPU in float64, written for this project from the module tree:
conv_pre; per stage leaky_relu(0.1), the transposed convolution, the mean over the residual blocks; leaky_relu(0.01), conv_post,
tanh.  dtype None: the weights are folded in float64 (g v / ||v||) and nothing is rounded -- what the reference module computes
after .double() and remove_weight_norm().  dtype fp16 / bf16: the weights are the fp32 fold rounded to the type (what the vocoder
holds), the spectrogram is rounded to the type; emulate=True additionally rounds wherever HifiGanVocoder writes a 16-bit tensor:
every convolution's output after its epilogue (bias, the block's residual, the running sum over the blocks, the division) and
the operand a = leaky_relu(x) of every convolution (an fp32 product rounded to the type).

fill_state: every state tensor from numpy's RandomState (a stream that is stable across versions and machines): weight_v ~
gain * N(0, 1 / fan_in), weight_g = ||v|| (so the folded weight is v), bias ~ 0.1 N(0, 1); fan_in = ksize * C of a convolution,
(k / u) * Cin of a transposed one (the taps that reach one output sample); conv_post takes post_gain.
"""
import collections

import numpy as np
import torch

from deeplearningexamples_amd.functional import fold_weight_norm
from deeplearningexamples_amd.hifigan.model import HifiGanGenerator, check_config, layers

SMALL_CONFIG = {"upsample_rates": [8, 2, 2], "upsample_kernel_sizes": [16, 4, 4], "upsample_initial_channel": 64, "resblock": "1",
                "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
# chosen on the CPU so that the float64 forward alone keeps max |activation| < 16384 and the audio RMS inside [0.05, 0.9]
# (tests/test_gpu_hifigan_infer.py asserts both): small / V1 configuration: RMS 0.17 / 0.23, max |activation| 17 / 19
GAIN, POST_GAIN = 1.2, 0.3
SEED = 20240


def fill_state(config, seed=SEED, gain=GAIN, post_gain=POST_GAIN):
    """-> OrderedDict name -> fp32 tensor, the reference's names and shapes."""
    rs = np.random.RandomState(seed)
    out = collections.OrderedDict()
    for l in layers(config):
        if l.kind == "conv":
            shape, fan = (l.cout, l.cin, l.ksize), l.ksize * l.cin
        else:
            shape, fan = (l.cin, l.cout, l.ksize), l.ksize * l.cin / l.stride
        g = post_gain if l.name == "conv_post" else gain
        v = torch.from_numpy(rs.standard_normal(shape) * g * fan ** -0.5).float()
        out[l.name + ".bias"] = torch.from_numpy(rs.standard_normal((l.cout,)) * 0.1).float()
        out[l.name + ".weight_g"] = torch.linalg.vector_norm(v, 2, dim=(1, 2), keepdim=True)
        out[l.name + ".weight_v"] = v
    return out


def make_mel(shape, seed=SEED + 1):
    """A spectrogram N(0, 1): conv_pre's output then has the scale of its weights."""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).float()


def folded64(model, dtype):
    """name -> (weight float64 in torch's layout, bias float64)."""
    out = {}
    for l in model.layers:
        if dtype is None:
            v, g = model.params[l.name + ".weight_v"].double(), model.params[l.name + ".weight_g"].double()
            w = v * (g / v.pow(2).sum((1, 2), keepdim=True).sqrt()) if l.name not in model.folded else model.folded[l.name].double()
        else:
            w = model.folded_weight(l.name).to(dtype).double()
        out[l.name] = (w.cpu(), model.params[l.name + ".bias"].double().cpu())
    return out


def forward64(model, mel, dtype=None, emulate=False):
    """model: a HifiGanGenerator; mel [B, 80, T] -> (audio float64 [B, T * hop], max |activation| over every tensor the vocoder
    writes in 16 bits: conv_pre's output, each upsampled tensor, each pair's intermediate and sum, each running sum)."""
    f = torch.nn.functional
    cfg = check_config(model.cfg)
    assert not (emulate and dtype is None)
    w = folded64(model, dtype)
    rnd = (lambda x: x.float().to(dtype).double()) if emulate else (lambda x: x)

    def act(x, slope):
        if emulate:                                                      # the contract: fl32(float(x) * slope) rounded to the type
            return torch.where(x < 0, (x.float() * slope).to(dtype).double(), x)
        return torch.where(x < 0, x * slope, x)

    def conv(x, name, dilation=1):
        wt, b = w[name]
        return f.conv1d(x, wt, b, 1, (wt.shape[2] - 1) // 2 * dilation, dilation)
    peak = 0.0
    nk = len(cfg["resblock_kernel_sizes"])
    with torch.no_grad():
        x = mel.cpu().double() if dtype is None else mel.cpu().float().to(dtype).double()
        x = rnd(conv(x, "conv_pre"))
        peak = max(peak, float(x.abs().max()))
        for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            wt, b = w["ups.%d" % i]
            x = rnd(f.conv_transpose1d(act(x, 0.1), wt, b, u, (k - u) // 2))
            peak = max(peak, float(x.abs().max()))
            xs = None
            for j, dil in enumerate(cfg["resblock_dilation_sizes"]):
                p = "resblocks.%d.%d." % (i, j)
                y = x
                n_pairs = 3 if cfg["resblock"] == "1" else 2
                for n in range(n_pairs):
                    if cfg["resblock"] == "1":
                        xt = rnd(conv(act(y, 0.1), p + "convs1.%d" % n, dil[n]))
                        peak = max(peak, float(xt.abs().max()))
                        y_new = conv(act(xt, 0.1), p + "convs2.%d" % n) + y
                    else:
                        y_new = conv(act(y, 0.1), p + "convs.%d" % n, dil[n]) + y
                    if n < n_pairs - 1:
                        y = rnd(y_new)
                    else:                                                # the block's last launch: + running sum, x alpha, one rounding
                        tot = y_new if xs is None else y_new + xs
                        if j == nk - 1:
                            tot = tot * float(np.float32(1.0 / nk)) if emulate else tot / nk
                        xs = rnd(tot)
                    peak = max(peak, float(y_new.abs().max()), float(xs.abs().max()) if xs is not None else 0.0)
            x = xs
        x = conv(act(x, 0.01), "conv_post")
        return torch.tanh(x)[:, 0], peak


def build_model(config, state=None, device="cpu"):
    m = HifiGanGenerator(config, device=device)
    m.load_state_dict(state if state is not None else fill_state(config))
    return m


__all__ = ["SMALL_CONFIG", "fill_state", "make_mel", "forward64", "build_model", "folded64", "fold_weight_norm"]
