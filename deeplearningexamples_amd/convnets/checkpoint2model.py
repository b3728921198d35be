"""Trainer checkpoint -> bare weights file: the reference's checkpoint2model.py
(Classification/ConvNets/checkpoint2model.py:18-45).  Host only.

    python -m deeplearningexamples_amd.convnets.checkpoint2model --checkpoint-path checkpoint_0089.pth.tar --weight-path rn50.pth

Writes the model's state dict (`module.` prefixes stripped) as --pretrained-from-file of classify / main reads it.  --ema takes the
averaged model a --use-ema run saved (`state_dict_ema`, training.py:194-202) and fails when the checkpoint has none.
"""
import argparse

import torch


def add_parser_arguments(parser):
    parser.add_argument("--checkpoint-path", metavar="<path>", required=True, help="checkpoint filename")
    parser.add_argument("--weight-path", metavar="<path>", required=True, help="name of file in which to store weights")
    parser.add_argument("--ema", action="store_true", default=False)
    return parser


def main(argv=None):
    args = add_parser_arguments(argparse.ArgumentParser(description="ResNet-50 checkpoint to weights file")).parse_args(argv)
    from .infer import state_from_checkpoint
    checkpoint = torch.load(args.checkpoint_path, map_location=torch.device("cpu"), weights_only=False)
    try:
        state = state_from_checkpoint(checkpoint, ema=args.ema)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.checkpoint_path, e))
    if isinstance(checkpoint, dict) and "best_prec1" in checkpoint:
        print("Loaded model, acc : %s" % checkpoint["best_prec1"])
    torch.save({k: v.detach().cpu() for k, v in state.items()}, args.weight_path)


if __name__ == "__main__":
    main()
