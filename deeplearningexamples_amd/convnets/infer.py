"""ResNet-50 inference on the gfx950 library: images -> logits / top-k, the forward the reference serves from classify.py and
main.py --evaluate (Classification/ConvNets/classify.py:119-144, image_classification/training.py:98-105 under model.eval()).

ResNetTrainer.infer (the validation pass of training) needs a whole trainer and runs every conv + BatchNorm unit as two launches:
the convolution writes a 16-bit t, dle_bn_fwd_apply reads it (and the residual) back.  In evaluation mode BatchNorm is a
per-channel affine map with constant coefficients, so here it sits in the convolution's epilogue, on the fp32 accumulator
(functional.conv2d_fwd_affine): one launch per unit, the activation written once and rounded once.  The weights are the
training path's 16-bit KRSC copies, unmodified -- the coefficients stay fp32 (a folded 16-bit weight would overflow where
running_var is tiny).

One stream: image layout pass -> stem convolution -> affine + ReLU + max pooling -> 52 fused units (conv1, conv2: affine + ReLU;
downsample: affine; conv3: affine + residual + ReLU) -> average pooling -> fc.  graphs=True keeps one captured graph (a single
chain) and one static input buffer per input shape; the logits of a call then live in a buffer the classifier owns: copy them
before the next call at that shape.

ResNeXtClassifier (below) serves ResNeXt101-32x4d and SE-ResNeXt101-32x4d on the same stem, 1x1 units, pooling and fc, with the
grouped 3x3 kernel and the squeeze-and-excitation launches in the block.
"""
import functools

import torch

from .. import functional as F
from ..utils.frontend import GraphCache, require_16bit
from ..utils.state import fold_bn, strip_module_prefix
from .resnet import ConvBN, ResNet50
from .resnext import CARDINALITY, ResNeXt101, state_has_se

# Units routed back to the two-launch form (convolution, then the stand-alone BatchNorm-apply): (kernel size, stride, C, Ko).
# The place to put a unit whose fused launch measures slower than the pair; tools/rn50_infer_perf.py times whole networks only, so
# no unit has been measured on its own and none is listed (DESIGN.md section 4h has the whole-network table).
TWO_LAUNCH_UNITS = frozenset()


def state_from_checkpoint(obj, ema=False):
    """The model's state dict out of what torch.load returned: the trainer's checkpoint_*.pth.tar (`state_dict`, or the averaged
    model `state_dict_ema` with ema=True), or a bare state dict; `module.` prefixes (DistributedDataParallel) are stripped."""
    if not isinstance(obj, dict):
        raise ValueError("not a checkpoint: expected a dict, got %s" % type(obj).__name__)
    if ema:
        keys = [k for k in ("state_dict_ema", "ema_state_dict") if k in obj]
        if not keys:
            raise ValueError("this checkpoint holds no averaged model (state_dict_ema): it was not trained with --use-ema")
        state = obj[keys[0]]
    else:
        state = obj.get("state_dict", obj)
    return strip_module_prefix(state)


def affine_relu_maxpool(t, scale, shift, zeros, ones):
    """maxpool3x3/2/pad1(relu(scale[c] * t + shift[c])) of the stem's 16-bit NHWC convolution output in one pass (H, W even):
    dle_bn_relu_maxpool_fwd, the training forward's kernel, with (mean, rstd, gamma, beta) = (zeros, scale, ones, shift) -- it forms
    rstd * gamma = scale and beta - mean * scale = shift exactly.  zeros / ones: constant fp32 [C] tensors the caller keeps (nothing
    is filled per call).  (The kernel also writes the argmax and keep bits training needs.)"""
    return F.bn_relu_maxpool_fwd(t, zeros, scale, ones, shift)[0]


class _Unit:
    """One conv + BatchNorm unit as the kernels read it: the 16-bit KRSC weight and the fp32 affine coefficients."""
    __slots__ = ("w16", "scale", "shift", "stride", "pad", "relu", "two_launch", "ones", "zeros")


def pack_unit(u, dtype, dev):
    """A conv + BatchNorm pair (conv, bn, k, stride, pad, relu: a resnet.ConvBN or anything shaped like it) -> _Unit on `dev`."""
    w = u.conv.weight.data
    ko, ci, r, s = w.shape
    cp = (ci + 7) // 8 * 8                # (the stem's 3 channels, padded for the generic convolution route)
    o = _Unit()
    o.w16 = torch.zeros((ko, r, s, cp), dtype=dtype, device=dev)
    F.cast_rows(w.permute(0, 2, 3, 1).reshape(ko * r * s, ci), dtype, cols_out=cp, out=o.w16.view(ko * r * s, cp))
    o.scale, o.shift = fold_bn(u.bn.weight.data, u.bn.bias.data, u.bn.running_mean, u.bn.running_var, u.bn.eps)
    o.stride, o.pad, o.relu = u.stride, u.pad, u.relu
    o.two_launch = (u.k, u.stride, ci, ko) in TWO_LAUNCH_UNITS
    # what the kernels of the training forward take as (mean, rstd, gamma, beta): (0, scale, 1, shift) -- the stem's pooling pass
    # (affine_relu_maxpool) and the stand-alone apply of a two-launch unit
    o.ones, o.zeros = torch.ones_like(o.scale), torch.zeros_like(o.scale)
    return o


@functools.lru_cache(maxsize=None)
def _mean_std_255(dev):
    """ImageNet's channel means and deviations on the 0..255 scale, one pair of fp32 [3] tensors per device."""
    from .dataloaders import IMAGENET_MEAN, IMAGENET_STD
    return torch.tensor(IMAGENET_MEAN, device=dev) * 255.0, torch.tensor(IMAGENET_STD, device=dev) * 255.0


def images_nhwc(images, c_padded, dtype):
    """NCHW images on the GPU -> 16-bit NHWC with the channels zero-padded to c_padded: fp32 images as they are, uint8 images
    normalised on the way (one launch either way)."""
    if images.dtype == torch.uint8:
        mean, std = _mean_std_255(images.device)
        return F.u8_nchw_normalize_nhwc(images, mean, std, dtype, c_padded)
    return F.nchw_to_nhwc(images, dtype, c_padded)


class ResNet50Classifier:
    def __init__(self, model, dtype=torch.bfloat16, device=None, graphs=False):
        """model: a ResNet50 (left untouched; nothing of it is referenced afterwards) or its state dict (any device; `module.`
        prefixes allowed).  dtype: torch.float16 or torch.bfloat16.  graphs: replay one captured graph per input shape."""
        require_16bit(dtype, "ResNet50Classifier")
        if not isinstance(model, ResNet50):
            state = state_from_checkpoint(model)
            dev = torch.device(device if device is not None else "cuda")
            module = ResNet50(num_classes=state["fc.weight"].shape[0], device=dev)
            module.load_state_dict(state)
            model = module
        self._init_common(model.fc, dtype, graphs)
        stem, blocks = model.units()
        with torch.no_grad():
            self.stem = self._unit(stem)
            self.stem_w2 = F.stem_pack_weight(model.conv1.weight.data, dtype)
            self.blocks = [tuple(self._unit(u) if u is not None else None for u in blk) for blk in blocks]

    def _init_common(self, fc, dtype, graphs):
        """What the three classifiers keep of the last layer `fc`, and their graph cache."""
        self.dev, self.dtype = fc.weight.device, dtype
        self.num_classes = fc.weight.shape[0]
        with torch.no_grad():
            self.fc_w16 = F.cast(fc.weight.data, dtype)
            self.fc_bias = fc.bias.data.float().clone()
        self._graphs = GraphCache(graphs)     # (input shape, input dtype) -> GraphedStep

    def _unit(self, u):
        return pack_unit(u, self.dtype, self.dev)

    @classmethod
    def from_checkpoint(cls, path, ema=False, **kw):
        """path: the trainer's checkpoint_*.pth.tar (ema=True: its averaged model), the file checkpoint2model writes, or any
        saved state dict."""
        obj = torch.load(path, map_location="cpu", weights_only=False)
        return cls(state_from_checkpoint(obj, ema=ema), **kw)

    # ------------------------------------------------------------------ the chain
    def _run(self, u, x, residual=None):
        if u.two_launch:
            t = F.conv2d_fwd(x, u.w16, u.stride, u.pad)
            return F.bn_fwd_apply(t, u.zeros, u.scale, u.ones, u.shift, residual=residual, relu=u.relu, want_mask=False)[0]
        return F.conv2d_fwd_affine(x, u.w16, u.scale, u.shift, u.stride, u.pad, residual=residual, relu=u.relu)

    def _stem(self, images):
        """-> the pooled 16-bit NHWC activation [N, H/4, W/4, 64]."""
        h, w = images.shape[-2:]
        p, q = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        stem4 = w <= 224 and p % 2 == 0 and q % 2 == 0
        x = images_nhwc(images, 4 if stem4 else 8, self.dtype)
        u = self.stem
        if stem4:
            # the stem's own kernel without statistics, then affine + ReLU + 3x3/2 max pooling in one pass: the 112x112x64
            # activation is written once
            t = F.stem_conv_fwd(x, self.stem_w2, want_stats=False)[0]
            return affine_relu_maxpool(t, u.scale, u.shift, u.zeros, u.ones)
        # images wider than 224 pixels / odd stem output: the generic convolution on the 8-channel image, then the pooling
        return F.maxpool_fwd(F.conv2d_fwd_affine(x, u.w16, u.scale, u.shift, 2, 3, relu=True))[0]

    def _forward(self, images):
        h = self._stem(images)
        for (u1, u2, u3, ud) in self.blocks:
            res = self._run(ud, h) if ud is not None else h
            h = self._run(u3, self._run(u2, self._run(u1, h)), residual=res)
        return self._fc(F.avgpool_fwd(h))

    def _fc(self, pooled):
        return F.gemm(pooled, self.fc_w16, pooled.shape[0], self.fc_w16.shape[0], self.fc_w16.shape[1], True, True,
                      out_dtype=torch.float32, bias=self.fc_bias)

    def logits(self, images):
        """images: fp32 (or uint8, normalised on the way in) NCHW, contiguous or channels_last -> fp32 logits [N, classes]."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError("%s: images must be [N, 3, H, W] (got %s)" % (type(self).__name__, tuple(images.shape)))
        if images.dtype not in (torch.float32, torch.uint8):
            raise ValueError("%s: fp32 or uint8 images (got %s)" % (type(self).__name__, images.dtype))
        if images.device != self.dev:
            images = images.to(self.dev)
        if not images.is_contiguous():
            images = images.contiguous()          # --memory-format nhwc loaders hand over channels_last tensors
        with torch.no_grad():
            return self._graphs.run((tuple(images.shape), images.dtype), self._forward, images)

    def predict(self, images, topk=5):
        """-> (softmax probabilities [N, classes] fp32, the indices [N, topk] of the most probable classes, most probable first)."""
        probs = torch.softmax(self.logits(images), dim=1)
        return probs, torch.topk(probs, min(topk, probs.shape[1]), dim=1).indices


class _Block:
    """One (SE-)ResNeXt bottleneck as the kernels read it."""
    __slots__ = ("u1", "u3", "ud", "w2", "scale2", "shift2", "stride", "se")


class ResNeXtClassifier(ResNet50Classifier):
    """ResNeXt101-32x4d / SE-ResNeXt101-32x4d inference (models/resnet.py:412-458): ResNet50Classifier's stem, 1x1 units, pooling and
    fc around the grouped 3x3 kernel (functional.conv2d_grouped_fwd_affine) and, for the SE variant, the two squeeze-and-excitation
    launches.  Per block: downsample (affine) on the first block of a stage, conv1 (affine + ReLU), the grouped conv2 (affine +
    ReLU), then conv3 with the residual and the ReLU in its epilogue -- or, with SE, conv3 (affine only), se_gate, se_apply
    (gate, residual, ReLU).  At 224 x 224: 33 x 3 + 4 convolution launches and at most 66 SE launches between the stem and the
    average pooling.  Grouped weights are packed [Ko, 3, 3, Cg] once here; SE weights stay fp32."""

    def __init__(self, model, dtype=torch.bfloat16, device=None, graphs=False):
        """model: a ResNeXt101 (left untouched) or a state dict of either architecture (any device; `module.` prefixes allowed; the
        SE variant is recognised by its squeeze weights)."""
        require_16bit(dtype, "ResNeXtClassifier")
        if not isinstance(model, ResNeXt101):
            state = state_from_checkpoint(model)
            dev = torch.device(device if device is not None else "cuda")
            module = ResNeXt101(num_classes=state["fc.weight"].shape[0], se=state_has_se(state), device=dev)
            module.load_state_dict(state)
            model = module
        self._init_common(model.fc, dtype, graphs)
        self.se = model.se
        with torch.no_grad():
            self.stem = self._unit(ConvBN(model.conv1, model.bn1, "conv1", "bn1", relu=True))
            self.stem_w2 = F.stem_pack_weight(model.conv1.weight.data, dtype)
            self.blocks = [self._block(blk) for blk in model.bottlenecks()]

    def _block(self, blk):
        b = _Block()
        b.u1 = self._unit(ConvBN(blk.conv1, blk.bn1, "conv1", "bn1", relu=True))
        # conv3 carries the residual add and the last ReLU in its epilogue; with SE both move to se_apply
        b.u3 = self._unit(ConvBN(blk.conv3, blk.bn3, "conv3", "bn3", relu=blk.squeeze is None))
        b.ud = None
        if blk.downsample is not None:
            b.ud = self._unit(ConvBN(blk.downsample[0], blk.downsample[1], "downsample.0", "downsample.1", relu=False))
        b.w2 = F.pack_grouped_weight(blk.conv2.weight.data, self.dtype)
        b.scale2, b.shift2 = fold_bn(blk.bn2.weight.data, blk.bn2.bias.data, blk.bn2.running_mean, blk.bn2.running_var, blk.bn2.eps)
        b.stride = blk.conv2.stride[0]
        b.se = None
        if blk.squeeze is not None:
            sq, ex = blk.squeeze.squeeze, blk.squeeze.expand
            b.se = tuple(t.data.float().contiguous().clone() for t in (sq.weight, sq.bias, ex.weight, ex.bias))
        return b

    def _forward(self, images):
        h = self._stem(images)
        for b in self.blocks:
            res = self._run(b.ud, h) if b.ud is not None else h
            t = self._run(b.u1, h)
            t = F.conv2d_grouped_fwd_affine(t, b.w2, b.scale2, b.shift2, CARDINALITY, b.stride, relu=True)
            if b.se is None:
                h = self._run(b.u3, t, residual=res)
            else:
                t = self._run(b.u3, t)
                h = F.se_apply(t, F.se_gate(t, *b.se), residual=res, relu=True)
        return self._fc(F.avgpool_fwd(h))

    def eval_step(self, images, target):
        """-> (loss [1] (plain cross entropy, like ResNetTrainer.eval_step), fp32 logits)."""
        logits = self.logits(images)
        if target.device != self.dev:
            target = target.to(self.dev)
        loss, _ = F.softmax_xent(logits, target, smoothing=0.0)
        return loss, logits


class _MBConv:
    """One MBConv block as the kernels read it."""
    __slots__ = ("expand", "w_dw", "scale_dw", "shift_dw", "stride", "in_act", "se", "proj", "residual")


class EfficientNetClassifier(ResNet50Classifier):
    """EfficientNet-B0..B7 / wide-SE inference (models/efficientnet.py:175-310, :384-452) around the depthwise kernel
    (functional.dwconv2d_act_fwd).  SiLU moves to the consumer: a unit the reference follows with SiLU runs
    with relu=False and writes its BatchNorm output, rounded once; whoever reads that tensor applies the SiLU while staging it and
    rounds the value to 16 bits, as the reference's SiLU writes a 16-bit tensor.  Per block: expand 1x1 (affine; absent at expansion
    1), the depthwise unit (input SiLU, affine, SiLU, SE pool partials), se_gate_act (SiLU hidden layer), se_apply, project 1x1
    (affine + residual where stride == 1 and in == out).  Stem: the 3x3 / 2 convolution on the 8-channel image; tail: features 1x1
    (affine), SiLU + average pooling, fc.  efficientnet.EffNetArch.launch_count() launches: 83 for b0, 162 for b4."""

    def __init__(self, model, dtype=torch.bfloat16, device=None, graphs=False):
        """model: an efficientnet.EfficientNet (left untouched) or a state dict / checkpoint dict of any architecture of the family
        (any device; `module.` prefixes and the published files' `layerN.` spelling allowed; original versus wide-SE is recognised
        from the squeeze weights' shapes)."""
        from . import efficientnet as E
        require_16bit(dtype, "EfficientNetClassifier")
        if not isinstance(model, E.EfficientNet):
            state = E.remap_ngc(state_from_checkpoint(model))
            dev = torch.device(device if device is not None else "cuda")
            module = E.build(E.arch_from_state(state), num_classes=state["classifier.fc.weight"].shape[0], device=dev)
            module.load_state_dict(state)
            model = module
        self._init_common(model.classifier.fc, dtype, graphs)
        self.arch = model.arch
        with torch.no_grad():
            self.stem = self._cb(model.stem)
            self.blocks = [self._block(blk, first=i == 0) for i, blk in enumerate(model.mbconv_blocks())]
            self.features = self._cb(model.features)

    def _cb(self, seq):
        """A conv + BatchNorm pair of the module tree -> _Unit, never with a ReLU: the SiLU behind it is its reader's."""
        return self._unit(ConvBN(seq.conv, seq.bn, "conv", "bn", relu=False))

    def _block(self, blk, first):
        b = _MBConv()
        b.expand = self._cb(blk.expand) if blk.expand is not None else None
        # the depthwise unit applies the SiLU of the unit it reads: the expand unit's, or the stem's for the network's first block;
        # a later block without an expand unit reads a projection, which has no activation
        b.in_act = b.expand is not None or first
        b.w_dw = F.pack_depthwise_weight(blk.depsep.conv.weight.data, self.dtype)
        bn = blk.depsep.bn
        b.scale_dw, b.shift_dw = fold_bn(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps)
        b.stride = blk.stride
        b.se = tuple(t.data.float().contiguous().clone() for t in (blk.se.squeeze.weight, blk.se.squeeze.bias, blk.se.expand.weight,
                                                                   blk.se.expand.bias))
        b.proj = self._cb(blk.proj)
        b.residual = blk.residual
        return b

    def _forward(self, images):
        h = self._run(self.stem, images_nhwc(images, 8, self.dtype))
        for b in self.blocks:
            t = h if b.expand is None else self._run(b.expand, h)
            t, pool = F.dwconv2d_act_fwd(t, b.w_dw, b.scale_dw, b.shift_dw, b.stride, in_act=b.in_act, out_act=True, pool=True)
            gate = F.se_gate_act(pool, 1.0 / (t.shape[1] * t.shape[2]), *b.se, act="silu")
            t = F.se_apply(t, gate, residual=None, relu=False)
            h = self._run(b.proj, t, residual=h if b.residual else None)
        return self._fc(F.silu_avgpool_fwd(self._run(self.features, h)))

    eval_step = ResNeXtClassifier.eval_step
