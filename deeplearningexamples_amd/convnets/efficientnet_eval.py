"""Evaluation entry point for EfficientNet on MI355X with the reference's command line.

Mirrors Classification/ConvNets/main.py --arch efficientnet-* --evaluate (flags :89-356, the validation pass of
image_classification/training.py:257-311) on convnets.infer.EfficientNetClassifier:
    python -m deeplearningexamples_amd.convnets.efficientnet_eval --arch efficientnet-b0 --amp --batch-size 256 \
        --pretrained-from-file nvidia_efficientnet-b0_210412.pth --data-backend pytorch /data/imagenet
The flags are convnets.main's; --arch takes the EfficientNet names (default efficientnet-b0), --image-size defaults to the
architecture's own size.  The family is inference-only here: --evaluate is implied and the training flags (optimizer, schedule, EMA,
augmentation, epochs) are parsed and ignored.  Reports val.top1 / val.top5 / val.loss through dllogger, as convnets.main does.
"""
import argparse
import os

import torch

from . import efficientnet as E
from .main import add_parser_arguments, evaluate_classifier


def parser():
    p = add_parser_arguments(argparse.ArgumentParser(description="EfficientNet evaluation on MI355X"))
    for a in p._actions:
        if a.dest == "arch":
            a.choices, a.default = list(E.ARCHS) + list(E.QUANT_ARCHS), "efficientnet-b0"
            a.help = "efficientnet-b0..b7 or efficientnet-widese-b0..b7 (evaluation only)"
        elif a.dest == "image_size":
            a.default, a.help = None, "default: the architecture's own size (224 for b0 ... 600 for b7)"
    p.add_argument("--trt", metavar="True|False", default=False, type=lambda s: str(s).lower() in ("1", "true", "yes"),
                   help="the reference's TensorRT-friendly module variants: not built")
    return p


def parse_args(argv=None):
    args = parser().parse_args(argv)
    if args.arch in E.QUANT_ARCHS:
        raise SystemExit("--arch %s: the quantised architectures need pytorch_quantization, which is not part of this path" % args.arch)
    if args.trt:
        raise SystemExit("--trt True: the TensorRT module variants are not built; the kernels run the plain architecture")
    if args.data_backend.startswith("dali"):
        raise SystemExit("--data-backend %s: DALI is not part of this path; use pytorch or synthetic" % args.data_backend)
    if not args.amp:
        raise SystemExit("this path computes in 16 bits: pass --amp (the reference's fp32 / TF32 recipes are not built)")
    args.evaluate = True
    if args.image_size is None:
        args.image_size = E.ARCHS[args.arch].default_image_size
    return args


def main(argv=None):
    from .infer import EfficientNetClassifier
    args = parse_args(argv)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16

    def make(device):
        path = args.pretrained_from_file or args.resume
        if not path:
            return EfficientNetClassifier(E.build(args.arch, num_classes=args.num_classes, device=device), dtype=dtype)
        if not os.path.isfile(path):
            raise SystemExit("=> no checkpoint found at '%s'" % path)
        return EfficientNetClassifier.from_checkpoint(path, dtype=dtype, device=device)
    return evaluate_classifier(args, make)


if __name__ == "__main__":
    main()
