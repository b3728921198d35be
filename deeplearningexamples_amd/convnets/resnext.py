"""ResNeXt101-32x4d and SE-ResNeXt101-32x4d: parameter containers with the reference's module tree / state_dict names.

Mirrors (Classification/ConvNets/image_classification/):
    models/resnet.py:107-175   Bottleneck with cardinality 32 (1x1 -> grouped 3x3(stride) -> 1x1, BN after each) and, for the SE
                               variant, `out = residual + out * squeeze(out)` before the last ReLU
    models/resnet.py:177-204   SEBottleneck (se_squeeze = 16: the HIDDEN WIDTH handed straight to nn.Linear(in_channels, squeeze))
    models/common.py:146-164   SqueezeAndExcitation (squeeze / expand Linear layers)
    models/resnet.py:412-458   the two architectures: layers [3, 4, 23, 3], widths [128, 256, 512, 1024], expansion 2
The stem, the downsample placement and the strides are ResNet50's (convnets/resnet.py).  These architectures are inference-only
here (convnets/infer.py: ResNeXtClassifier); the module owns the parameters under the reference's names and has no forward.
"""
import torch
from torch import nn

from .resnet import _bn, _conv

ARCHS = {"resnext101-32x4d": False, "se-resnext101-32x4d": True}          # name -> squeeze-and-excitation
LAYERS, WIDTHS, EXPANSION, CARDINALITY, SE_SQUEEZE = [3, 4, 23, 3], [128, 256, 512, 1024], 2, 32, 16


def _grouped_conv(planes, stride, device):
    m = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, groups=CARDINALITY, bias=False, device=device)
    nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
    return m


class SqueezeAndExcitation(nn.Module):
    def __init__(self, channels, squeeze, device):
        super().__init__()
        self.squeeze = nn.Linear(channels, squeeze, device=device)
        self.expand = nn.Linear(squeeze, channels, device=device)


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample, se, device, last_bn_0_init=False):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 1, 1, device)
        self.bn1 = _bn(planes, device)
        self.conv2 = _grouped_conv(planes, stride, device)
        self.bn2 = _bn(planes, device)
        self.conv3 = _conv(planes, planes * EXPANSION, 1, 1, device)
        self.bn3 = _bn(planes * EXPANSION, device, zero_init=last_bn_0_init)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.squeeze = SqueezeAndExcitation(planes * EXPANSION, SE_SQUEEZE, device) if se else None


class ResNeXt101(nn.Module):
    def __init__(self, num_classes=1000, se=False, last_bn_0_init=False, device="cuda"):
        super().__init__()
        self.se = bool(se)
        self.conv1 = _conv(3, 64, 7, 2, device)
        self.bn1 = _bn(64, device)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = 64
        layers = []
        for i, (w, n) in enumerate(zip(WIDTHS, LAYERS)):
            blocks = []
            for b in range(n):
                stride = (1 if i == 0 else 2) if b == 0 else 1
                down = None
                if b == 0:
                    down = nn.Sequential(_conv(inplanes, w * EXPANSION, 1, stride, device), _bn(w * EXPANSION, device))
                blocks.append(Bottleneck(inplanes, w, stride, down, self.se, device, last_bn_0_init))
                inplanes = w * EXPANSION
            layers.append(nn.Sequential(*blocks))
        self.layers = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(WIDTHS[-1] * EXPANSION, num_classes, device=device)

    def bottlenecks(self):
        return [blk for layer in self.layers for blk in layer]


def build(arch, num_classes=1000, last_bn_0_init=False, device="cuda"):
    """arch: "resnext101-32x4d" or "se-resnext101-32x4d"."""
    if arch not in ARCHS:
        raise ValueError("unknown architecture %r (one of %s)" % (arch, ", ".join(ARCHS)))
    return ResNeXt101(num_classes=num_classes, se=ARCHS[arch], last_bn_0_init=last_bn_0_init, device=device)


def state_has_se(state):
    """Whether a state dict (reference names) is the SE variant's."""
    return any(k.endswith(".squeeze.squeeze.weight") for k in state)
