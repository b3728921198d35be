"""SSD300 (ResNet-50 backbone) as a host-side module tree with the reference's parameter names and shapes
(PyTorch/Detection/SSD/ssd/model.py:20-129), the default boxes (ssd/utils.py:224-290) and the checkpoint forms of ssd/main.py:232-243.

The module holds parameters and states the network in plain torch (forward: the float reference of the tests, any dtype, any
device); inference on the library is ssd.infer.SSDDetector.  Only the resnet50 backbone is built: the reference's other backbones
are turned away.

Names.  `feature_extractor.feature_extractor` is the first seven children of a torchvision ResNet-50 -- conv1, bn1, relu, maxpool,
layer1, layer2, layer3 -- in an nn.Sequential, so the keys are feature_extractor.feature_extractor.{0,1,4,5,6}.* with torchvision's
bottleneck spelling (conv1/bn1/conv2/bn2/conv3/bn3/downsample.0/downsample.1); layer3's first block runs conv1, conv2 and
downsample.0 at stride 1 (model.py:44-48), which keeps the 38 x 38 map.  `width` divides every channel count (1: the published
network; 8: the trunk is [128, 64, 64, 32, 32, 32] with 32 / 16 middle channels -- a network whose float64 forward takes seconds).
"""
import itertools
from math import sqrt

import numpy as np
import torch
import torch.nn as nn

from ..utils.state import strip_module_prefix

BACKBONES = ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")
NUM_DEFAULTS = (4, 6, 6, 6, 4, 4)
LABEL_NUM = 81


def reject_backbone(name):
    """The one-line rejection of everything but resnet50 (the constructor's and the command line's)."""
    if name != "resnet50":
        raise ValueError("SSD300: only the resnet50 backbone is built (got %r; resnet18/34/101/152 are out of scope)" % (name,))


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride sits on conv2), by its parameter names."""

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + idt)


def _layer(inplanes, planes, blocks, stride):
    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    mods = [Bottleneck(inplanes, planes, stride, down)]
    mods += [Bottleneck(planes * 4, planes, 1, None) for _ in range(1, blocks)]
    return nn.Sequential(*mods)


class ResNet(nn.Module):
    """model.py:20-52: ResNet-50 cut after layer3, that stage at stride 1."""

    def __init__(self, backbone="resnet50", width=1):
        super().__init__()
        reject_backbone(backbone)
        if width < 1 or 64 % width:
            raise ValueError("SSD300: width must divide 64 (got %r)" % (width,))
        c = 64 // width
        self.out_channels = [v // width for v in (1024, 512, 512, 256, 256, 256)]
        self.feature_extractor = nn.Sequential(
            nn.Conv2d(3, c, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
            _layer(c, c, 3, 1), _layer(4 * c, 2 * c, 4, 2), _layer(8 * c, 4 * c, 6, 1))

    def forward(self, x):
        return self.feature_extractor(x)


class SSD300(nn.Module):
    def __init__(self, backbone="resnet50", width=1, label_num=LABEL_NUM):
        super().__init__()
        self.feature_extractor = backbone if isinstance(backbone, ResNet) else ResNet(backbone, width)
        self.width = width
        self.label_num = label_num
        oc = self.feature_extractor.out_channels
        self.num_defaults = list(NUM_DEFAULTS)
        blocks = []
        for i, (cin, cout, mid) in enumerate(zip(oc[:-1], oc[1:], [v // width for v in (256, 256, 128, 128, 128)])):
            second = nn.Conv2d(mid, cout, 3, padding=1, stride=2, bias=False) if i < 3 else nn.Conv2d(mid, cout, 3, bias=False)
            blocks.append(nn.Sequential(nn.Conv2d(cin, mid, 1, bias=False), nn.BatchNorm2d(mid), nn.ReLU(inplace=True),
                                        second, nn.BatchNorm2d(cout), nn.ReLU(inplace=True)))
        self.additional_blocks = nn.ModuleList(blocks)
        self.loc = nn.ModuleList([nn.Conv2d(c, nd * 4, 3, padding=1) for nd, c in zip(self.num_defaults, oc)])
        self.conf = nn.ModuleList([nn.Conv2d(c, nd * label_num, 3, padding=1) for nd, c in zip(self.num_defaults, oc)])
        for layer in [*self.additional_blocks, *self.loc, *self.conf]:
            for p in layer.parameters():
                if p.dim() > 1:
                    nn.init.xavier_uniform_(p)

    def features(self, x):
        """The six detection feeds."""
        x = self.feature_extractor(x)
        feeds = [x]
        for blk in self.additional_blocks:
            x = blk(x)
            feeds.append(x)
        return feeds

    def forward(self, x):
        """-> (ploc [N, 4, B], plabel [N, label_num, B]): every head's NCHW output reshaped and concatenated (bbox_view)."""
        n = x.shape[0]
        locs, confs = [], []
        for s, l, c in zip(self.features(x), self.loc, self.conf):
            locs.append(l(s).reshape(n, 4, -1))
            confs.append(c(s).reshape(n, self.label_num, -1))
        return torch.cat(locs, 2).contiguous(), torch.cat(confs, 2).contiguous()


class DefaultBoxes:
    """utils.py:224-280, the same float64 arithmetic and the same single rounding to fp32; feat_size is free."""

    def __init__(self, fig_size, feat_size, steps, scales, aspect_ratios, scale_xy=0.1, scale_wh=0.2):
        self.fig_size, self.feat_size, self.steps, self.scales, self.aspect_ratios = fig_size, feat_size, steps, scales, aspect_ratios
        self.scale_xy, self.scale_wh = scale_xy, scale_wh
        fk = fig_size / np.array(steps)
        boxes = []
        for idx, sfeat in enumerate(feat_size):
            sk1, sk2 = scales[idx] / fig_size, scales[idx + 1] / fig_size
            sk3 = sqrt(sk1 * sk2)
            sizes = [(sk1, sk1), (sk3, sk3)]
            for alpha in aspect_ratios[idx]:
                w, h = sk1 * sqrt(alpha), sk1 / sqrt(alpha)
                sizes += [(w, h), (h, w)]
            for w, h in sizes:
                for i, j in itertools.product(range(sfeat), repeat=2):
                    boxes.append(((j + 0.5) / fk[idx], (i + 0.5) / fk[idx], w, h))
        self.num_defaults = [2 + 2 * len(a) for a in aspect_ratios]
        self.dboxes = torch.tensor(boxes, dtype=torch.float).clamp_(min=0, max=1)
        d = self.dboxes
        self.dboxes_ltrb = torch.stack((d[:, 0] - 0.5 * d[:, 2], d[:, 1] - 0.5 * d[:, 3], d[:, 0] + 0.5 * d[:, 2],
                                        d[:, 1] + 0.5 * d[:, 3]), dim=1)

    def __call__(self, order="ltrb"):
        if order == "ltrb":
            return self.dboxes_ltrb
        if order == "xywh":
            return self.dboxes
        raise ValueError("DefaultBoxes: order is 'ltrb' or 'xywh'")


def dboxes300_coco():
    return DefaultBoxes(300, [38, 19, 10, 5, 3, 1], [8, 16, 32, 64, 100, 300], [21, 45, 99, 153, 207, 261, 315],
                        [[2], [2, 3], [2, 3], [2, 3], [2], [2]])


def state_from_checkpoint(obj):
    """The model's state dict out of what torch.load returned: the reference's checkpoint {'model': state_dict, ...}
    (main.py:232-243), or a bare state dict; `module.` prefixes (DistributedDataParallel) are stripped."""
    if not isinstance(obj, dict):
        raise ValueError("not a checkpoint: expected a dict, got %s" % type(obj).__name__)
    state = obj["model"] if "model" in obj and isinstance(obj["model"], dict) else obj
    return strip_module_prefix(state)


def width_from_state(state):
    return 64 // state["feature_extractor.feature_extractor.0.weight"].shape[0]
