"""Reference statements for the SSD300 tests (CPU, torch): the box decode, softmax, per-class top-k, greedy non-maximum suppression
and per-image selection of Detection/SSD/ssd/utils.py:127-221 restated so that they return INDICES (box index, label) and run in
whatever float type their inputs have -- float64 as the reference of the decode and of the whole detector, fp32 as the reference
algorithm the NMS / selection kernels must reproduce bit for bit; the decision margins of a case; a float64 forward of the host
model with and without the emulated 16-bit roundings; the seeded input generator of the recorded cases; and the small
torchvision-shaped ResNet-50 that tools/make_ssd_fixture.py hands to the reference's ssd/model.py in place of torchvision's.

Order rules (the reference's sort leaves equal scores open): inside a class the higher score first, then the LOWER box index; in
the final list the higher score, then the lower label, then the lower box index.
"""
import copy

import numpy as np
import torch
import torch.nn as nn

U32 = 2.0 ** -24          # fp32 unit roundoff
THRESHOLD, MAX_NUM = 0.05, 200
PROB_MARGIN, IOU_MARGIN = 1e-5, 1e-4      # absolute on probabilities and score gaps; relative to `criteria` on the IoU

TINY = dict(fig_size=300, feat_size=[3, 2, 1], steps=[100, 150, 300], scales=[60, 120, 200, 280], aspect_ratios=[[2], [2, 3], [2]])
TINY_LABELS = 5
# seeds of the recorded cases: the first ones whose float64 run meets the margin condition (tests/test_ssd_host.py asserts it)
FULL_SEED, TINY_SEED = 2, 1


# ------------------------------------------------------------------ the torchvision-shaped stand-in backbone
class TvBottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + idt)


class TvResNet50(nn.Module):
    """Children in torchvision's order: conv1, bn1, relu, maxpool, layer1..layer4, avgpool, fc."""

    def __init__(self, base=64):
        super().__init__()
        self.conv1 = nn.Conv2d(3, base, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(base)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = base
        for i, (mult, blocks) in enumerate(zip((1, 2, 4, 8), (3, 4, 6, 3))):
            planes, stride = base * mult, 1 if i == 0 else 2
            down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            mods = [TvBottleneck(inplanes, planes, stride, down)] + [TvBottleneck(planes * 4, planes) for _ in range(1, blocks)]
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*mods))
            inplanes = planes * 4
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(inplanes, 1000)


def resnet50(weights=None, **kw):
    return TvResNet50()


# ------------------------------------------------------------------ seeded inputs of the recorded cases
def case_inputs(dboxes_xywh, n, num_labels, seed, big_class=True):
    """(ploc [n,4,B], plabel [n,L,B]) fp32 numpy: background-dominated logits (background 8 +- 0.1, every other label -2 +- 0.5: far
    below the threshold); per image a handful of classes boosted on a cluster of overlapping boxes (the 12 boxes whose centres are
    nearest to a random point), the boosted logits an evenly spaced ladder in random order so that scores are well separated; with
    big_class, image 0 carries one class with 260 candidates spread over the first map (more than max_num = 200, mostly disjoint
    boxes); at least one label is never boosted."""
    d = np.asarray(dboxes_xywh, dtype=np.float64)
    b = d.shape[0]
    rng = np.random.RandomState(seed)
    ploc = 0.5 * rng.standard_normal((n, 4, b))
    plabel = rng.normal(-2.0, 0.5, (n, num_labels, b))
    plabel[:, 0] = 8.0 + 0.1 * rng.standard_normal((n, b))
    boosted = rng.choice(np.arange(1, num_labels), size=min(6, num_labels - 2), replace=False)
    for i in range(n):
        for c in boosted:
            centre = rng.uniform(0.25, 0.75, 2)
            members = np.argsort(np.abs(d[:, :2] - centre).max(1), kind="stable")[:min(12, b // 4)]
            ladder = np.linspace(5.6, 12.0, len(members))
            rng.shuffle(ladder)
            plabel[i, c, members] = ladder
    if big_class:
        fs = int(round(np.sqrt(np.sum(np.isclose(d[:, 2], d[0, 2]) & np.isclose(d[:, 3], d[0, 3])))))     # first map, anchor 0
        lattice = np.asarray([h * fs + w for h in range(0, fs, 2) for w in range(0, fs, 2)])
        members = rng.choice(lattice, size=260, replace=False)
        ladder = np.linspace(5.6, 12.0, len(members))
        rng.shuffle(ladder)
        plabel[0, boosted[0], members] = ladder
        ploc[0][:, members] *= 0.3
    return ploc.astype(np.float32), plabel.astype(np.float32)


# ------------------------------------------------------------------ decode, IoU, NMS, selection (dtype-preserving)
def decode_ref(ploc, plabel, dboxes_xywh, scale_xy=0.1, scale_wh=0.2):
    """Encoder.scale_back_batch: ploc [N,4,B], plabel [N,L,B] -> (boxes [N,B,4] ltrb, probs [N,L,B]) in ploc's dtype."""
    d = dboxes_xywh.to(ploc.dtype)
    loc = ploc.permute(0, 2, 1)
    xy = scale_xy * loc[:, :, :2] * d[None, :, 2:] + d[None, :, :2]
    wh = (scale_wh * loc[:, :, 2:]).exp() * d[None, :, 2:]
    boxes = torch.cat((xy - 0.5 * wh, xy + 0.5 * wh), dim=2)
    return boxes, torch.softmax(plabel, dim=1)


def iou_ref(b1, b2):
    """calc_iou_tensor of b1 [K,4] against one box b2 [4], its operations in its order."""
    lt = torch.max(b1[:, :2], b2[None, :2])
    rb = torch.min(b1[:, 2:], b2[None, 2:])
    delta = rb - lt
    delta = torch.where(delta < 0, torch.zeros_like(delta), delta)
    inter = delta[:, 0] * delta[:, 1]
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[2] - b2[0]) * (b2[3] - b2[1])
    return inter / (a1 + a2 - inter)


def new_margins():
    return {"prob": float("inf"), "iou": float("inf"), "rank": float("inf"), "final": float("inf"), "order": float("inf")}


def _low(m, key, value):
    if m is not None and value == value:
        m[key] = min(m[key], float(value))


def nms_ref(boxes, score, criteria, threshold=THRESHOLD, max_num=MAX_NUM, margins=None):
    """The class loop's body of decode_single on boxes [B,4] and one class's score [B] -> LongTensor of the kept box indices, best
    first.  margins: |score - threshold|, the neighbour gaps of the best max_num + 1 candidates, |iou - criteria| / criteria over
    every pair the sweep compares."""
    if score.numel():
        _low(margins, "prob", (score.double() - threshold).abs().min())
    cand = torch.nonzero(score > threshold).flatten()
    if cand.numel() == 0:
        return cand
    order = torch.sort(score[cand], descending=True, stable=True).indices
    if margins is not None and cand.numel() > 1:
        top = score[cand][order][:max_num + 1].double()
        _low(margins, "rank", (top[:-1] - top[1:]).min())
    order = cand[order][:max_num]
    k = order.numel()
    bx = boxes[order]
    alive = torch.ones(k, dtype=torch.bool, device=boxes.device)
    kept = []
    for i in range(k):
        if not alive[i]:
            continue
        kept.append(int(order[i]))
        rest = torch.nonzero(alive[i + 1:]).flatten() + i + 1
        if rest.numel() == 0:
            continue
        iou = iou_ref(bx[rest], bx[i])
        if margins is not None:
            rel = ((iou.double() - criteria).abs() / criteria)
            rel = rel[rel == rel]
            if rel.numel():
                _low(margins, "iou", rel.min())
        alive[rest[~(iou < criteria)]] = False
    return torch.tensor(kept, dtype=torch.long, device=boxes.device)


def detect_ref(boxes, probs, criteria, max_output, threshold=THRESHOLD, max_num=MAX_NUM, margins=None):
    """decode_single on boxes [B,4] and probs [L,B] (one image) -> (idx, label, score) best first, idx / label LongTensors; plus the
    per-class kept lists [(label, idx LongTensor)]."""
    idx, lab, sc, per_class = [], [], [], []
    for label in range(1, probs.shape[0]):
        kept = nms_ref(boxes, probs[label], criteria, threshold, max_num, margins)
        per_class.append((label, kept))
        idx.append(kept)
        lab.append(torch.full((kept.numel(),), label, dtype=torch.long, device=boxes.device))
        sc.append(probs[label][kept])
    idx, lab, sc = torch.cat(idx), torch.cat(lab), torch.cat(sc)
    # higher score, then lower label, then lower index: the lists are already (label, rank) ordered; a stable sort keeps label order,
    # and inside a label equal scores are in index order
    order = torch.sort(sc, descending=True, stable=True).indices
    if margins is not None and order.numel() > 1:
        s = sc[order].double()
        gaps = s[:-1] - s[1:]
        _low(margins, "order", gaps[:max_output].min())
        lo, hi = max(0, max_output - 2), max_output + 1
        if gaps[lo:hi].numel():
            _low(margins, "final", gaps[lo:hi].min())
    order = order[:max_output]
    return idx[order], lab[order], sc[order], per_class


def margins_ok(m):
    return m["prob"] >= PROB_MARGIN and m["iou"] >= IOU_MARGIN and m["rank"] >= PROB_MARGIN and m["final"] >= PROB_MARGIN


# ------------------------------------------------------------------ the host model in float64
def randomise(model, seed, head_gain=1.0, background_bias=0.0):
    """Random BatchNorm statistics and affine parameters (bn3's gamma small, as tests/test_gpu_resnext_infer.py does, so that 13
    residual blocks stay in range), head biases N(0, 0.1) with background_bias added on the background label's channels, head
    weights scaled by head_gain."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
                gamma = torch.rand(c, generator=g)
                m.weight.copy_(gamma * 0.25 + 0.125 if name.endswith("bn3") else gamma + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.2)
        for nd, loc, conf in zip(model.num_defaults, model.loc, model.conf):
            loc.bias.copy_(torch.randn(loc.bias.shape, generator=g) * 0.1)
            conf.bias.copy_(torch.randn(conf.bias.shape, generator=g) * 0.1)
            conf.bias[:nd] += background_bias           # conf channel c is label c // nd: the first nd channels are the background
            conf.weight.mul_(head_gain)
            loc.weight.mul_(head_gain)
    return model


def calibrate_heads(model, images, dtype, seed, share=0.01, spread=12.0):
    """Shifts the confidence biases so that the network DETECTS something on `images` with few close decisions.  A random network's
    class logits vary far more between channels than over the pixels of one channel, so without this either nothing passes the
    threshold or whole channels do (thousands of candidates at probability ~1, score gaps of an ulp).  For every confidence channel
    c (label c // nd >= 1, anchor c % nd) the filter and its bias are scaled so that the channel's float64 logits have standard
    deviation `spread` over the images' pixels, and the largest value of logit_c - logit_background is then moved to a target:
    log-odds -2.94 + U(0.3, 3) for a random `share` of the channels (a peak of probability 0.07 .. 0.5 with a few neighbouring pixels
    above the threshold), -12 for the others (never a candidate)."""
    heads, _ = forward64(model, images, dtype, emulate=False)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for nd, conf, (_, c64) in zip(model.num_defaults, model.conf, heads):
            nch = c64.shape[1]
            std = c64[:, nd:].std(dim=(0, 2, 3)) if c64[:, 0].numel() > 1 else torch.ones(nch - nd, dtype=torch.float64)
            s = (spread / std.clamp_min(1e-3)).clamp(0.05, 200.0)
            conf.weight[nd:] *= s[:, None, None, None].to(conf.weight.dtype)
            conf.bias[nd:] *= s.to(conf.bias.dtype)
            diff = c64[:, nd:] * s[None, :, None, None] - c64[:, :nd].repeat(1, nch // nd - 1, 1, 1)
            peak = diff.amax(dim=(0, 2, 3))
            chosen = torch.rand(nch - nd, generator=g) < share
            target = torch.where(chosen, -2.94 + 0.3 + 2.7 * torch.rand(nch - nd, generator=g), torch.full((nch - nd,), -12.0))
            conf.bias[nd:] += (target.double() - peak).to(conf.bias.dtype)
    return model


def forward64(model, images, dtype, emulate):
    """float64 CPU forward under eval() over the 16-bit-rounded weights and images -> the six (loc, conf) NCHW head outputs and the
    largest |activation|.  emulate: round to `dtype` where the detector writes a 16-bit tensor (after every unit and every head)."""
    f = torch.nn.functional
    m = copy.deepcopy(model).cpu().double().eval()
    r16 = lambda w: w.detach().float().to(dtype).double()
    rnd = (lambda x: x.float().to(dtype).double()) if emulate else (lambda x: x)
    bn = lambda x, b: f.batch_norm(x, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)
    conv = lambda x, c: f.conv2d(x, r16(c.weight), None, c.stride, c.padding)
    fe = m.feature_extractor.feature_extractor
    peak = 0.0
    with torch.no_grad():
        x = images.cpu().to(dtype).double()
        x = f.max_pool2d(rnd(torch.relu(bn(conv(x, fe[0]), fe[1]))), 3, 2, 1)
        for layer in (fe[4], fe[5], fe[6]):
            for blk in layer:
                idn = x if blk.downsample is None else rnd(bn(conv(x, blk.downsample[0]), blk.downsample[1]))
                o = rnd(torch.relu(bn(conv(x, blk.conv1), blk.bn1)))
                o = rnd(torch.relu(bn(conv(o, blk.conv2), blk.bn2)))
                x = rnd(torch.relu(bn(conv(o, blk.conv3), blk.bn3) + idn))
                peak = max(peak, float(x.abs().max()))
        feeds = [x]
        for blk in m.additional_blocks:
            x = rnd(torch.relu(bn(conv(x, blk[0]), blk[1])))
            x = rnd(torch.relu(bn(conv(x, blk[3]), blk[4])))
            peak = max(peak, float(x.abs().max()))
            feeds.append(x)
        heads = []
        for s, l, c in zip(feeds, m.loc, m.conf):
            heads.append((rnd(conv(s, l) + l.bias[None, :, None, None]), rnd(conv(s, c) + c.bias[None, :, None, None])))
    return heads, peak


def bbox_view(heads, label_num):
    """SSD300.bbox_view on the NCHW head outputs -> (ploc [N,4,B], plabel [N,L,B])."""
    n = heads[0][0].shape[0]
    return (torch.cat([l.reshape(n, 4, -1) for l, _ in heads], 2).contiguous(),
            torch.cat([c.reshape(n, label_num, -1) for _, c in heads], 2).contiguous())


def decode_bar(ploc, plabel, dboxes_xywh, scale_xy=0.1, scale_wh=0.2):
    """Per-element bars on the fp32 decode of fp32-exact inputs against decode_ref in float64.
    boxes: each coordinate is a chain of at most 5 fp32 operations on magnitudes bounded by |xy| + |wh| (the scale product, the
    product with d, the sum; expf within 2 ulp, its argument's rounding carried through the exponential: |arg| u exp(arg)) ->
    (6 + |arg|) u (|xy| + wh) with u = 2^-24, doubled for slack in the constants.
    probs: the subtraction of the maximum is rounded to 1 u of |c - max|, which the exponential carries as |c - max| u e, in the
    numerator and in the terms of the sum; expf within 2 ulp = 4 u, again on both; the L-term sum (L - 1) u; the division 1 u
    -> (L + 8 + 2 |c - max|) u p."""
    d = dboxes_xywh.double()
    loc = ploc.double().permute(0, 2, 1)
    arg = (scale_wh * loc[:, :, 2:]).abs()
    wh = (scale_wh * loc[:, :, 2:]).exp() * d[None, :, 2:]
    xy_mag = (scale_xy * loc[:, :, :2]).abs() * d[None, :, 2:] + d[None, :, :2].abs()
    one = 2 * (6 + arg) * U32 * (xy_mag + wh)
    box_bar = torch.cat((one, one), dim=2)
    c = plabel.double()
    dist = (c - c.max(dim=1, keepdim=True).values).abs()
    prob_bar = (plabel.shape[1] + 8 + 2 * dist) * U32 * torch.softmax(c, dim=1) + 2.0 ** -149
    return box_bar, prob_bar
