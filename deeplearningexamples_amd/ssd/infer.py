"""SSD300 inference on the gfx950 library: images -> detections (PyTorch/Detection/SSD/ssd/model.py:117-129 under model.eval(),
ssd/utils.py:127-221, the loop of ssd/evaluate.py:47-67).

One stream, one launch per unit: image layout pass -> the 7x7 stem on the 8-channel image (the generic convolution, as
ResNet50Classifier does for images wider than 224) -> max pooling -> 13 bottlenecks of 3 fused units + 3 downsample units (layer1,
layer2, layer3; layer4 is cut) -> 5 additional blocks of 2 units -> 6 head launches on the concatenated [loc; conf] weights (scale 1,
shift = bias, output channels zero-padded to a multiple of HEAD_PAD) = 1 + 1 + 39 + 3 + 10 + 6 = 60 network launches behind the
layout pass, then the three post-processing launches of csrc/ssd.hip (decode, per-class NMS, per-image selection).  Nothing is read
back inside detect(); decode_batch() reads one packed tensor per batch.
"""
import types

import torch

from .. import functional as F
from ..convnets.infer import _Unit, images_nhwc, pack_unit
from ..utils.frontend import GraphCache, require_16bit
from . import model as M

# Output channels of a head launch are zero-padded to a multiple of this: 340 / 510 become 384 / 512, which puts the 3x3 / pad 1 heads
# on the halo-tile kernel.  8 (344 / 512, the convolution's minimum) measured slower: the six launches take 0.84x the time at batch
# 32 and 0.96x at batch 1 with 64 (tools/ssd_infer_perf.py)
HEAD_PAD = 64


class SSDDetector:
    def __init__(self, model, dtype=torch.bfloat16, device=None, graphs=False, dboxes=None, head_pad=None):
        """model: an ssd.model.SSD300 (left untouched) or a state dict / the reference's checkpoint dict (any device; `module.`
        prefixes allowed; the width is read from the stem).  dtype: torch.float16 or torch.bfloat16.  graphs: replay one captured
        graph per (input shape, call).  dboxes: the DefaultBoxes of the geometry (default: dboxes300_coco)."""
        require_16bit(dtype, "SSDDetector")
        if not isinstance(model, M.SSD300):
            state = M.state_from_checkpoint(model)
            module = M.SSD300("resnet50", width=M.width_from_state(state), label_num=state["conf.0.weight"].shape[0] // M.NUM_DEFAULTS[0])
            module.load_state_dict(state)
            model = module.to(torch.device(device if device is not None else "cuda"))
        self.dev = model.loc[0].weight.device
        self.dtype = dtype
        self.label_num = model.label_num
        self.num_defaults = list(model.num_defaults)
        self.head_pad = int(head_pad or HEAD_PAD)
        fe = model.feature_extractor.feature_extractor
        with torch.no_grad():
            self.stem = self._cb(fe[0], fe[1], True)
            self.blocks = []
            for layer in (fe[4], fe[5], fe[6]):
                for blk in layer:
                    ud = None if blk.downsample is None else self._cb(blk.downsample[0], blk.downsample[1], False)
                    # conv3 carries the residual add and the block's last ReLU in its epilogue
                    self.blocks.append((self._cb(blk.conv1, blk.bn1, True), self._cb(blk.conv2, blk.bn2, True),
                                        self._cb(blk.conv3, blk.bn3, True), ud))
            self.extra = [(self._cb(b[0], b[1], True), self._cb(b[3], b[4], True)) for b in model.additional_blocks]
            self.heads = [self._head(l, c) for l, c in zip(model.loc, model.conf)]
            # per map (nd, loc offset, conf offset) inside the head launch's output pitch
            self.geom = [(nd, 0, 4 * nd) for nd in self.num_defaults]
        self.dboxes = dboxes if dboxes is not None else M.dboxes300_coco()
        self.dboxes_xywh = self.dboxes("xywh").to(self.dev).contiguous()
        self.scale_xy, self.scale_wh = self.dboxes.scale_xy, self.dboxes.scale_wh
        self._graphs = GraphCache(graphs)     # (call, input shape, input dtype, the call's scalars) -> GraphedStep

    def _cb(self, conv, bn, relu):
        u = types.SimpleNamespace(conv=conv, bn=bn, stride=conv.stride[0], pad=conv.padding[0], relu=relu, k=conv.kernel_size[0])
        return pack_unit(u, self.dtype, self.dev)

    def _head(self, loc, conf):
        """One unit for both heads of a map: rows [0, 4 nd) are loc's filters, [4 nd, 4 nd + L nd) conf's, then zero rows."""
        w = torch.cat((loc.weight.data, conf.weight.data), 0)
        b = torch.cat((loc.bias.data, conf.bias.data), 0).float()
        ko, ci = w.shape[:2]
        kp = (ko + self.head_pad - 1) // self.head_pad * self.head_pad
        o = _Unit()
        o.w16 = torch.zeros((kp, 3, 3, ci), dtype=self.dtype, device=self.dev)
        F.cast_rows(w.permute(0, 2, 3, 1).reshape(ko * 9, ci), self.dtype, out=o.w16.view(kp * 9, ci)[:ko * 9])
        o.scale = torch.ones(kp, dtype=torch.float32, device=self.dev)
        o.shift = torch.zeros(kp, dtype=torch.float32, device=self.dev)
        o.shift[:ko] = b
        o.stride, o.pad, o.relu, o.two_launch = 1, 1, False, False
        o.ones = o.zeros = None
        return o

    @classmethod
    def from_checkpoint(cls, path, **kw):
        """path: the reference's checkpoint ({'model': state_dict, ...}) or any saved state dict."""
        return cls(torch.load(path, map_location="cpu", weights_only=False), **kw)

    # ------------------------------------------------------------------ the chain
    @staticmethod
    def _run(u, x, residual=None):
        return F.conv2d_fwd_affine(x, u.w16, u.scale, u.shift, u.stride, u.pad, residual=residual, relu=u.relu)

    def _heads(self, images):
        """-> the six 16-bit NHWC head tensors [N, fs, fs, pad(nd * (4 + L))]."""
        h = F.maxpool_fwd(self._run(self.stem, images_nhwc(images, 8, self.dtype)))[0]
        for (u1, u2, u3, ud) in self.blocks:
            res = self._run(ud, h) if ud is not None else h
            h = self._run(u3, self._run(u2, self._run(u1, h)), residual=res)
        feeds = [h]
        for (a, b) in self.extra:
            h = self._run(b, self._run(a, h))
            feeds.append(h)
        return tuple(self._run(u, f) for u, f in zip(self.heads, feeds))

    def _detect(self, images, criteria, max_output):
        heads = self._heads(images)
        boxes, probs = F.ssd_decode(heads, self.geom, self.dboxes_xywh, self.label_num, self.scale_xy, self.scale_wh)
        kept = F.ssd_nms(boxes, probs, criteria=criteria, threshold=0.05, max_num=200)
        det_boxes, det_label, det_score, det_idx, det_count = F.ssd_select(boxes, *kept, max_output=max_output)
        return det_boxes, det_label, det_score, det_count, det_idx

    def _check(self, images):
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError("SSDDetector: images must be [N, 3, H, W] (got %s)" % (tuple(images.shape),))
        if images.dtype not in (torch.float32, torch.uint8):
            raise ValueError("SSDDetector: fp32 (normalised) or uint8 images (got %s)" % images.dtype)
        if images.device != self.dev:
            images = images.to(self.dev)
        return images if images.is_contiguous() else images.contiguous()

    def _call(self, tag, fn, images, *scalars):
        images = self._check(images)
        with torch.no_grad():
            return self._graphs.run((tag, tuple(images.shape), images.dtype) + scalars, lambda im: fn(im, *scalars), images)

    def head_outputs(self, images):
        """The six head tensors as the kernels wrote them (16-bit NHWC, zero-padded channels behind nd * (4 + L))."""
        return self._call("heads", self._heads, images)

    def raw(self, images):
        """-> (ploc [N, 4, B], plabel [N, L, B]) in the detector's dtype: the reference forward's outputs, gathered from the head
        tensors with the reference's reshape (not on the hot path)."""
        locs, confs = [], []
        for t, nd in zip(self.head_outputs(images), self.num_defaults):
            n = t.shape[0]
            nchw = t.permute(0, 3, 1, 2)
            locs.append(nchw[:, :4 * nd].reshape(n, 4, -1))
            confs.append(nchw[:, 4 * nd:(4 + self.label_num) * nd].reshape(n, self.label_num, -1))
        return torch.cat(locs, 2).contiguous(), torch.cat(confs, 2).contiguous()

    def detect(self, images, criteria=0.5, max_output=200, with_index=False):
        """-> (boxes [N, max_output, 4] fp32 ltrb, labels [N, max_output] int32, scores [N, max_output] fp32, counts [N] int32), best
        first, rows past the count zero; device tensors, no host read.  with_index: the default-box indices [N, max_output] as well.
        With graphs=True the tensors are the graph's static outputs: copy them before the next call."""
        out = self._call("detect", self._detect, images, float(criteria), int(max_output))
        return out if with_index else out[:4]

    def decode_batch(self, images, criteria=0.45, max_output=200):
        """The reference's Encoder.decode_batch on the network's outputs: a list of (bboxes [k,4], labels [k] int64, scores [k]) CPU
        tensors per image in the reference's ascending-score order.  One host read per batch."""
        boxes, labels, scores, _ = self.detect(images, criteria, max_output)
        packed = torch.cat((boxes, labels.unsqueeze(2).float(), scores.unsqueeze(2)), dim=2).cpu()      # the host read
        out = []
        for row in packed:
            k = int((row[:, 4] > 0).sum())             # labels are 1..L-1; rows past the count are zero
            r = row[:k].flip(0)
            out.append((r[:, :4].contiguous(), r[:, 4].long(), r[:, 5].contiguous()))
        return out
