"""The HiFi-GAN generator's parameters under the reference's names (SpeechSynthesis/HiFiGAN/hifigan/models.py:140-232).

A container, not a module: it holds the tensors of `Generator(conf).state_dict()` -- conv_pre, ups.N, resblocks.N.M.convs1.J /
convs2.J (resblock '1') or resblocks.N.M.convs.J (resblock '2'), conv_post; each weight-normed: weight_g, weight_v, bias -- and
loads what the reference's checkpoints hold.  The forward lives in hifigan/infer.py.
"""
import collections

import torch

from ..utils.state import ParamTable, strip_module_prefix

N_MEL = 80
LRELU_SLOPE = 0.1
CONFIG_KEYS = ("upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock", "resblock_kernel_sizes",
               "resblock_dilation_sizes")
V1_CONFIG = {"upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
             "resblock": "1", "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}

Layer = collections.namedtuple("Layer", "name kind cin cout ksize dilation stride")     # kind: "conv" or "up"


def check_config(config):
    cfg = {k: config[k] for k in CONFIG_KEYS if k in config}
    missing = [k for k in CONFIG_KEYS if k not in cfg]
    if missing:
        raise ValueError("HiFi-GAN config lacks %s" % ", ".join(missing))
    cfg["resblock"] = str(cfg["resblock"])
    if cfg["resblock"] not in ("1", "2"):
        raise ValueError("resblock must be '1' or '2' (got %r)" % (cfg["resblock"],))
    if len(cfg["upsample_rates"]) != len(cfg["upsample_kernel_sizes"]):
        raise ValueError("upsample_rates and upsample_kernel_sizes differ in length")
    if len(cfg["resblock_kernel_sizes"]) != len(cfg["resblock_dilation_sizes"]):
        raise ValueError("resblock_kernel_sizes and resblock_dilation_sizes differ in length")
    return cfg


def layers(config):
    """Every convolution of the generator in the reference's construction order: [Layer]."""
    cfg = check_config(config)
    c0 = cfg["upsample_initial_channel"]
    out = [Layer("conv_pre", "conv", N_MEL, c0, 7, 1, 1)]
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        out.append(Layer("ups.%d" % i, "up", c0 // 2 ** i, c0 // 2 ** (i + 1), k, 1, u))
    for i in range(len(cfg["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for j, (k, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            pre = "resblocks.%d.%d." % (i, j)
            if cfg["resblock"] == "1":
                for n, d in enumerate(dil[:3]):
                    out.append(Layer(pre + "convs1.%d" % n, "conv", ch, ch, k, d, 1))
                for n in range(3):
                    out.append(Layer(pre + "convs2.%d" % n, "conv", ch, ch, k, 1, 1))
            else:
                for n, d in enumerate(dil[:2]):
                    out.append(Layer(pre + "convs.%d" % n, "conv", ch, ch, k, d, 1))
    out.append(Layer("conv_post", "conv", ch, 1, 7, 1, 1))
    return out


def state_shapes(config):
    """name -> shape of Generator(config).state_dict(), in its order: the modules as Generator.__init__ registers them (conv_pre, ups,
    resblocks, conv_post), per weight-normed module bias, weight_g, weight_v (tests/test_hifigan_host.py compares the key lists)."""
    shapes = collections.OrderedDict()
    for l in layers(config):
        # Conv1d weight [out, in, k], g over dim 0 = out; ConvTranspose1d weight [in, out, k], g over dim 0 = in
        first, second = (l.cout, l.cin) if l.kind == "conv" else (l.cin, l.cout)
        shapes[l.name + ".bias"] = (l.cout,)
        shapes[l.name + ".weight_g"] = (first, 1, 1)
        shapes[l.name + ".weight_v"] = (first, second, l.ksize)
    return shapes


def normalize_keys(state):
    """`module.` prefixes stripped and the older flat `resblocks.N.` keys mapped to `resblocks.N//3.N%3.`, the constant 3 as in
    Generator.load_state_dict (models.py:182-206)."""
    out = collections.OrderedDict()
    for k, v in strip_module_prefix(state).items():
        if k.startswith("resblocks."):
            parts = k.split(".")
            if len(parts) == 5:
                n = int(parts[1])
                k = "resblocks.%d.%d.%s" % (n // 3, n % 3, ".".join(parts[2:]))
        out[k] = v
    return out


class HifiGanGenerator(ParamTable):
    """The generator's parameters as fp32 tensors on `device`: weight_g / weight_v / bias per layer, zero until loaded."""

    def __init__(self, config, device="cpu"):
        self.cfg = check_config(config)
        self.layers = layers(self.cfg)
        self.folded = {}                      # layer name -> folded fp32 weight, for a checkpoint saved after remove_weight_norm
        super().__init__(state_shapes(self.cfg), device)

    def load_state_dict(self, state):
        """The reference's generator state: weight-normed (weight_g + weight_v) or folded (`weight`, saved after
        remove_weight_norm: kept as it is, folded_weight() returns it), nested or flat resblock keys, `module.` prefixes,
        weights with a trailing unit dimension more or less (the reference's Conv1d / Conv2d fix-up)."""
        state = normalize_keys(state)
        want = self.shapes
        self.folded = {}
        seen = set()
        for k, v in state.items():
            base, _, leaf = k.rpartition(".")
            v = v.detach().to(self.device, torch.float32)
            if leaf == "weight" and base + ".weight_v" in want:
                shape = want[base + ".weight_v"]
                v = self._fit(v, shape, k)
                self.folded[base] = v.clone()
                seen.update((base + ".weight_v", base + ".weight_g"))
                continue
            if k not in want:
                raise KeyError("unexpected key %r in a HiFi-GAN generator state" % k)
            self.params[k] = self._fit(v, want[k], k).clone()
            seen.add(k)
        missing = [k for k in want if k not in seen]
        if missing:
            raise KeyError("HiFi-GAN generator state lacks %s" % ", ".join(missing[:8]))
        return self

    @staticmethod
    def _fit(v, shape, key):
        if v.dim() == len(shape) + 1 and v.shape[-1] == 1:
            v = v.squeeze(-1)
        elif v.dim() == len(shape) - 1:
            v = v.unsqueeze(-1)
        if tuple(v.shape) != tuple(shape):
            raise ValueError("%s: shape %s, expected %s" % (key, tuple(v.shape), tuple(shape)))
        return v

    def folded_weight(self, name):
        """fp32 weight of layer `name` in torch's layout: the checkpoint's folded tensor, or g v / ||v||."""
        from ..functional import fold_weight_norm
        if name in self.folded:
            return self.folded[name]
        return fold_weight_norm(self.params[name + ".weight_v"], self.params[name + ".weight_g"])
