"""Classify one image with ResNet-50 or SE-ResNeXt101-32x4d on the MI355X: the interface of the reference's classify.py
(Classification/ConvNets/classify.py:56-76,119-144) on convnets.infer.ResNet50Classifier / ResNeXtClassifier.

    python -m deeplearningexamples_amd.convnets.classify --image IMG --pretrained-from-file WEIGHTS [--amp-dtype fp16]

--arch, --image-size, --precision, --cpu, --image and the model's --pretrained-from-file are the reference's flags.  resnet50 and
se-resnext101-32x4d are built (plain resnext101-32x4d is evaluated through convnets.main --evaluate only); FP32 and --cpu are
parsed and rejected with a message.  --amp-dtype picks the 16-bit type (the reference's autocast is
fp16).  The image is decoded with PIL when it is installed; otherwise --image takes a uint8 HWC (or HW) array saved with
numpy.save, the pre-decoded form convnets/dataloaders.py reads.  Resize to image-size + 32, centre crop and mean / std
normalisation run on the device.  Class names come from --synset-mapping FILE (a JSON list, the layout of the reference's
LOC_synset_mapping.json); without it the class indices are printed.
"""
import argparse
import json

import numpy as np
import torch

ARCHS = ("resnet50", "resnext101-32x4d", "se-resnext101-32x4d", "efficientnet-b0", "efficientnet-b4", "efficientnet-widese-b0",
         "efficientnet-widese-b4", "efficientnet-quant-b0", "efficientnet-quant-b4")
BUILT = ("resnet50", "se-resnext101-32x4d")


def add_parser_arguments(parser):
    parser.add_argument("--image-size", default=224, type=int)
    parser.add_argument("--arch", "-a", metavar="ARCH", default="resnet50", choices=ARCHS,
                        help="model architecture: " + " | ".join(ARCHS) + " (default: resnet50; built: " + ", ".join(BUILT) + ")")
    parser.add_argument("--precision", metavar="PREC", default="AMP", choices=["AMP", "FP32"])
    parser.add_argument("--cpu", action="store_true", help="perform inference on CPU (not built)")
    parser.add_argument("--image", metavar="<path>", help="path to classified image")
    parser.add_argument("--pretrained-from-file", default=None, type=str, metavar="<path>",
                        help="weights: the file checkpoint2model writes, a saved state dict, or a trainer checkpoint")
    parser.add_argument("--amp-dtype", default="fp16", choices=["bf16", "fp16"])
    parser.add_argument("--synset-mapping", default=None, type=str, metavar="FILE", help="JSON list of class names")
    return parser


def reject_unbuilt(args):
    if args.arch == "resnext101-32x4d":
        raise SystemExit("--arch resnext101-32x4d: classify serves resnet50 and se-resnext101-32x4d; evaluate this one with "
                         "convnets.main --arch resnext101-32x4d --evaluate")
    if args.arch not in BUILT:
        raise SystemExit("--arch %s: only resnet50 and se-resnext101-32x4d are built on this path" % args.arch)
    if args.cpu:
        raise SystemExit("--cpu: the kernels run on the MI355X only; there is no CPU path")
    if args.precision != "AMP":
        raise SystemExit("this path computes in 16 bits: pass --precision AMP (the reference's fp32 / TF32 recipes are not built)")
    if not args.image:
        raise SystemExit("--image is required")


def read_image(path):
    """-> uint8 [H, W, 3] array.  PIL when it imports, else a numpy.save'd uint8 HWC / HW array."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and not path.endswith(".npy"):
        return np.asarray(Image.open(path).convert("RGB"))
    if not path.endswith(".npy"):
        raise SystemExit("PIL is not installed: --image takes a uint8 HWC array saved with numpy.save (.npy)")
    a = np.load(path)
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=-1)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise SystemExit("%s: expected a uint8 [H, W, 3] (or [H, W]) array, got %s %s" % (path, a.dtype, a.shape))
    return a


def preprocess(array, image_size, device):
    """transforms.Resize(image_size + 32) -> CenterCrop(image_size) -> ToTensor -> (x - mean) / std, on the device.
    -> fp32 [1, 3, image_size, image_size]."""
    from .dataloaders import IMAGENET_MEAN, IMAGENET_STD
    img = torch.from_numpy(np.ascontiguousarray(array)).to(device).permute(2, 0, 1).unsqueeze(0).float() / 255.0
    h, w = img.shape[-2:]
    s = image_size + 32
    rh, rw = (s, max(1, int(s * w / h))) if h <= w else (max(1, int(s * h / w)), s)     # the shorter side becomes s
    img = torch.nn.functional.interpolate(img, size=(rh, rw), mode="bilinear", antialias=True, align_corners=False)
    top, left = int(round((rh - image_size) / 2.0)), int(round((rw - image_size) / 2.0))
    img = img[:, :, top:top + image_size, left:left + image_size]
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    return ((img - mean) / std).contiguous()


def format_top5(path, probs, indices, names=None):
    """The lines the reference prints: the path, then `class: xx.x%` for the five most probable classes."""
    lines = [path]
    for i in indices:
        lines.append("%s: %.1f%%" % (names[int(i)] if names is not None else "class %d" % int(i), 100.0 * float(probs[int(i)])))
    return lines


def main(argv=None):
    args = add_parser_arguments(argparse.ArgumentParser(description="ResNet-50 image classification on MI355X")).parse_args(argv)
    reject_unbuilt(args)
    from .infer import ResNet50Classifier, ResNeXtClassifier
    from .resnet import ResNet50
    from .resnext import build as build_resnext
    device = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    names = json.load(open(args.synset_mapping)) if args.synset_mapping else None
    if args.arch != "resnet50":
        if args.pretrained_from_file:
            clf = ResNeXtClassifier.from_checkpoint(args.pretrained_from_file, dtype=dtype, device=device)
        else:
            clf = ResNeXtClassifier(build_resnext(args.arch, device=device), dtype=dtype)
    elif args.pretrained_from_file:
        clf = ResNet50Classifier.from_checkpoint(args.pretrained_from_file, dtype=dtype, device=device)
    else:
        clf = ResNet50Classifier(ResNet50(device=device), dtype=dtype)          # (random weights, as the reference without a file)
    if names is not None and len(names) != clf.num_classes:
        raise SystemExit("--synset-mapping holds %d names, the model has %d classes" % (len(names), clf.num_classes))
    probs, top = clf.predict(preprocess(read_image(args.image), args.image_size, device), topk=5)
    print("\n".join(format_top5(args.image, probs[0].cpu(), top[0].cpu(), names)))


if __name__ == "__main__":
    main()
