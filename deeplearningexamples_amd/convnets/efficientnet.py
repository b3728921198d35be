"""EfficientNet-B0..B7 and the wide-SE variants: parameter containers with the reference's module tree / state_dict names.

Mirrors (Classification/ConvNets/image_classification/):
    models/efficientnet.py:51-115    EffNetArch and its width / depth scaling (divisor 8, never more than 10 % down)
    models/efficientnet.py:175-310   EfficientNet: stem (3x3 / 2) -> layers of MBConv blocks -> features (1x1) -> pooling, fc
    models/efficientnet.py:384-452   MBConvBlock: expand 1x1 (absent at expansion 1) -> depthwise k x k -> SE -> project 1x1,
                                     `x + b` when stride == 1 and in == out; squeeze width = max(1, int(base * 0.25)) with base =
                                     the block's input channels (original_mbconv) or its hidden width (widese_mbconv)
    models/efficientnet.py:513-571   the b0 table, the b1..b7 scalings and the architecture names
    models/common.py:31-79           conv: padding int((k-1)/2), no bias; BatchNorm eps 1e-3; :123-128 SiLU; :146-164 SE
These architectures are inference-only here (convnets/infer.py: EfficientNetClassifier).  The module's forward is the plain torch
composition under model.eval() (StochasticDepthResidual = torch.add, dropout = identity): the tests' float reference.
"""
import math
from collections import OrderedDict
from dataclasses import dataclass, replace
from typing import Tuple

import torch
from torch import nn

BN_EPS = 1e-3


@dataclass(frozen=True)
class EffNetArch:
    widese: bool
    stem_channels: int
    feature_channels: int
    kernel: Tuple[int, ...]
    stride: Tuple[int, ...]
    num_repeat: Tuple[int, ...]
    expansion: Tuple[int, ...]
    channels: Tuple[int, ...]
    default_image_size: int
    squeeze_excitation_ratio: float = 0.25

    def scale(self, wc, dc, dis, divisor=8):
        def sw(c):
            c *= wc
            r = max(divisor, int(c + divisor / 2) // divisor * divisor)
            return r + divisor if r < 0.9 * c else r
        return replace(self, stem_channels=sw(self.stem_channels), feature_channels=sw(self.feature_channels),
                       num_repeat=tuple(int(math.ceil(r * dc)) for r in self.num_repeat),
                       channels=tuple(sw(c) for c in self.channels), default_image_size=dis)

    def blocks(self):
        """[(layer, block, kernel, stride, in channels, out channels, expansion)] in network order."""
        out, cin = [], self.stem_channels
        for i, (k, s, r, e, c) in enumerate(zip(self.kernel, self.stride, self.num_repeat, self.expansion, self.channels)):
            for j in range(r):
                out.append((i, j, k, s if j == 0 else 1, cin, c, e))
                cin = c
        return out

    def launch_count(self):
        """Kernel launches of EfficientNetClassifier behind the image preparation: the stem, per block (expand,) depthwise, gate,
        SE apply and project, then features, SiLU + pooling, fc."""
        return 1 + sum(4 if e == 1 else 5 for *_, e in self.blocks()) + 3


_B0 = EffNetArch(widese=False, stem_channels=32, feature_channels=1280, kernel=(3, 3, 5, 3, 5, 5, 3), stride=(1, 2, 2, 2, 1, 2, 1),
                 num_repeat=(1, 2, 2, 3, 3, 4, 1), expansion=(1, 6, 6, 6, 6, 6, 6), channels=(16, 24, 40, 80, 112, 192, 320),
                 default_image_size=224)
_SCALINGS = [(1, 1, 224), (1, 1.1, 240), (1.1, 1.2, 260), (1.2, 1.4, 300), (1.4, 1.8, 380), (1.6, 2.2, 456), (1.8, 2.6, 528),
             (2.0, 3.1, 600)]
ARCHS = {}
for _i, (_wc, _dc, _dis) in enumerate(_SCALINGS):
    ARCHS["efficientnet-b%d" % _i] = _B0 if _i == 0 else _B0.scale(_wc, _dc, _dis)
for _i in range(len(_SCALINGS)):
    ARCHS["efficientnet-widese-b%d" % _i] = replace(ARCHS["efficientnet-b%d" % _i], widese=True)
QUANT_ARCHS = tuple("efficientnet-quant-b%d" % i for i in range(8))


def _unit(cin, cout, k, stride, groups, device):
    conv = nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=(k - 1) // 2, groups=groups, bias=False, device=device)
    nn.init.kaiming_normal_(conv.weight, mode="fan_in", nonlinearity="relu")
    return nn.Sequential(OrderedDict([("conv", conv), ("bn", nn.BatchNorm2d(cout, eps=BN_EPS, momentum=0.01, device=device))]))


class SqueezeAndExcitation(nn.Module):
    def __init__(self, channels, squeeze, device):
        super().__init__()
        self.squeeze = nn.Linear(channels, squeeze, device=device)
        self.expand = nn.Linear(squeeze, channels, device=device)

    def forward(self, x):
        g = torch.sigmoid(self.expand(nn.functional.silu(self.squeeze(x.mean((2, 3))))))
        return g[:, :, None, None] * x


class MBConvBlock(nn.Module):
    def __init__(self, k, cin, cout, expansion, stride, se_ratio, widese, device):
        super().__init__()
        hidden = cin * expansion
        self.kernel, self.stride, self.residual = k, stride, stride == 1 and cin == cout
        self.expand = None if hidden == cin else _unit(cin, hidden, 1, 1, 1, device)
        self.depsep = _unit(hidden, hidden, k, stride, hidden, device)
        self.se = SqueezeAndExcitation(hidden, max(1, int((hidden if widese else cin) * se_ratio)), device)
        self.proj = _unit(hidden, cout, 1, 1, 1, device)

    def forward(self, x):
        t = x if self.expand is None else nn.functional.silu(self.expand(x))
        b = self.proj(self.se(nn.functional.silu(self.depsep(t))))
        return x + b if self.residual else b


class EfficientNet(nn.Module):
    def __init__(self, arch, num_classes=1000, device=None):
        super().__init__()
        self.arch = arch
        self.stem = _unit(3, arch.stem_channels, 3, 2, 1, device)
        layers = [OrderedDict() for _ in arch.kernel]
        for (i, j, k, s, cin, cout, e) in arch.blocks():
            layers[i]["block%d" % j] = MBConvBlock(k, cin, cout, e, s, arch.squeeze_excitation_ratio, arch.widese, device)
        self.layers = nn.Sequential(*[nn.Sequential(l) for l in layers])
        self.features = _unit(arch.channels[-1], arch.feature_channels, 1, 1, 1, device)
        self.classifier = nn.Sequential(OrderedDict([("fc", nn.Linear(arch.feature_channels, num_classes, device=device))]))

    def mbconv_blocks(self):
        return [blk for layer in self.layers for blk in layer]

    def forward(self, x):
        x = self.layers(nn.functional.silu(self.stem(x)))
        return self.classifier(nn.functional.silu(self.features(x)).mean((2, 3)))


def build(arch, num_classes=1000, device=None):
    """arch: a name of ARCHS (efficientnet-b0..b7, efficientnet-widese-b0..b7) or an EffNetArch."""
    if isinstance(arch, str):
        if arch in QUANT_ARCHS:
            raise ValueError("%s: the quantised architectures need pytorch_quantization, which is not part of this path" % arch)
        if arch not in ARCHS:
            raise ValueError("unknown architecture %r (one of %s)" % (arch, ", ".join(ARCHS)))
        arch = ARCHS[arch]
    return EfficientNet(arch, num_classes=num_classes, device=device)


def remap_ngc(state):
    """The published 20.12.0 / 21.03.0 checkpoints spell `layer{i+1}.` for `layers.{i}.` (EfficientNet.ngc_checkpoint_remap,
    models/efficientnet.py:360-378); other names pass through."""
    out = OrderedDict()
    for k, v in state.items():
        head, _, rest = k.partition(".")
        if head.startswith("layer") and head[5:].isdigit():
            k = "layers.%d.%s" % (int(head[5:]) - 1, rest)
        out[k] = v
    return out


def arch_from_state(state):
    """The EffNetArch a state dict (reference names) was built from: every width, kernel size, repeat count and the squeeze rule are
    read from the tensors' shapes; the strides are b0's schedule, which every published architecture shares."""
    nl = 1 + max(int(k.split(".")[1]) for k in state if k.startswith("layers."))
    if nl != len(_B0.stride):
        raise ValueError("not an EfficientNet state dict: %d layers (expected %d)" % (nl, len(_B0.stride)))
    stem = state["stem.conv.weight"].shape[0]
    kernel, repeat, expansion, channels, widese, cin = [], [], [], [], None, stem
    for i in range(nl):
        pre = "layers.%d." % i
        repeat.append(1 + max(int(k[len(pre) + 5:].split(".")[0]) for k in state if k.startswith(pre + "block")))
        dw = state[pre + "block0.depsep.conv.weight"]
        kernel.append(dw.shape[-1])
        expansion.append(dw.shape[0] // cin)
        channels.append(state[pre + "block0.proj.conv.weight"].shape[0])
        sq = state[pre + "block0.se.squeeze.weight"].shape[0]
        narrow, wide = max(1, int(cin * 0.25)), max(1, int(dw.shape[0] * 0.25))
        if narrow != wide:
            if sq not in (narrow, wide) or (widese is not None and widese != (sq == wide)):
                raise ValueError("layers.%d.block0.se.squeeze.weight: %d hidden units fit neither squeeze rule" % (i, sq))
            widese = sq == wide
        cin = channels[-1]
    size = next((a.default_image_size for a in ARCHS.values() if a.channels == tuple(channels) and a.num_repeat == tuple(repeat)), 224)
    return EffNetArch(widese=bool(widese), stem_channels=stem, feature_channels=state["features.conv.weight"].shape[0],
                      kernel=tuple(kernel), stride=_B0.stride, num_repeat=tuple(repeat), expansion=tuple(expansion),
                      channels=tuple(channels), default_image_size=size)
