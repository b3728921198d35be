"""Writes the nnU-Net fixtures under tests/golden/ from a checkout of the reference recipe (CPU only).  Recorded data only: results
of the reference's programs, never their text.

    python tools/make_nnunet_fixture.py --reference /path/to/DeepLearningExamples/PyTorch/Segmentation/nnUNet

  nnunet_unet3d.npz        float64 outputs of the reference's UNet3D (brats22_model.py) under eval() at the two geometries of
                           tests/_nnunet_ref.GEOMETRIES: three levels on a [1, 5, 8, 12, 16] input, two levels on [2, 5, 4, 4, 4]
  nnunet_state_dict.json   parameter names and shapes of UNet3D at six, three and two levels, in state_dict order
  nnunet_unet_params.json  what NNUnet.get_unet_params (nn_unet.py:139-159) returns for task 11 (config from
                           data_preprocessing/configs.py, --depth 5 --min_fmap 4)
  nnunet_cli_flags.json    flags, defaults and kinds of utils/args.py's parser

Weights are deeplearningexamples_amd.nnunet.model.seeded_state (values representable in fp16); none are committed.  UNet3D builds
its two deep-supervision heads from filters[1] and filters[2], so the class itself cannot be constructed with two levels: for that
geometry the heads (unused under eval()) are left out by a subclass that overrides get_deep_supervision_heads only.
nn_unet.py imports pytorch_lightning, apex, monai, DALI's loader and skimage at module level: they are stubbed in sys.modules; only
get_unet_params runs, on a stand-in `self`.
"""
import argparse
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def parser_flags(path):
    """(flag, default, action, type, nargs, choices) of every `arg(...)` call of utils/args.py, from its syntax tree."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and getattr(node.func, "id", "") == "arg" and node.args and isinstance(node.args[0], ast.Constant) \
                and str(node.args[0].value).startswith("--"):
            kw = {k.arg: k.value for k in node.keywords}
            lit = lambda k: ast.literal_eval(kw[k]) if k in kw else None
            action = lit("action")
            out.append({"flag": node.args[0].value, "default": False if action == "store_true" and "default" not in kw else lit("default"),
                        "action": action, "type": getattr(kw.get("type"), "id", None), "nargs": lit("nargs"), "choices": lit("choices")})
    return out


def stub_modules():
    def mod(name, **attrs):
        m = sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    ident = lambda f: f
    mod("pytorch_lightning", LightningModule=object)
    mod("pytorch_lightning.utilities", rank_zero_only=ident)
    mod("apex")
    mod("apex.optimizers", FusedAdam=object, FusedSGD=object)
    mod("data_loading")
    mod("data_loading.data_module", get_data_path=None, get_test_fnames=None)
    mod("monai")
    mod("monai.inferers", sliding_window_inference=None)
    mod("monai.networks")
    mod("monai.networks.nets", DynUNet=None)
    mod("nnunet.loss", Loss=None, LossBraTS=None)
    mod("nnunet.metrics", Dice=None)
    mod("skimage")
    mod("skimage.transform", resize=None)
    mod("utils.logger", DLLogger=None)
    mod("utils.utils", get_config_file=lambda args: args.config_dict, print0=print)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import torch
    from nnunet import brats22_model as B
    from deeplearningexamples_amd.nnunet import model as M
    from tests import _nnunet_ref as R
    os.makedirs(GOLDEN, exist_ok=True)

    class UNet3DNoHeads(B.UNet3D):
        def get_deep_supervision_heads(self):
            return torch.nn.ModuleList([])

    def build(levels):
        cls = B.UNet3D if levels >= 3 else UNet3DNoHeads
        return cls([[3, 3, 3]] * levels, [[1, 1, 1]] + [[2, 2, 2]] * (levels - 1))

    # 1. names and shapes
    json.dump({str(l): [[k, list(v.shape)] for k, v in build(l).state_dict().items()] for l in (6, 3, 2)},
              open(os.path.join(GOLDEN, "nnunet_state_dict.json"), "w"), indent=0)

    # 2. the float64 forward at the two geometries
    rec = {}
    for tag, (levels, shape, seed) in R.GEOMETRIES.items():
        net = build(levels)
        net.load_state_dict(M.seeded_state(levels, R.WEIGHT_SEED))
        net = net.double().eval()
        with torch.no_grad():
            out = net(R.seeded_input(shape, seed))
        assert out.dtype == torch.float64 and tuple(out.shape) == (shape[0], 3) + tuple(shape[2:])
        rec[tag] = out.numpy()
        print(tag, "logits: max |.| %.4f, std %.4f" % (float(out.abs().max()), float(out.std())))
    np.savez_compressed(os.path.join(GOLDEN, "nnunet_unet3d.npz"), weight_seed=R.WEIGHT_SEED, **rec)

    # 3. get_unet_params for task 11
    from data_preprocessing import configs
    stub_modules()
    from nnunet import nn_unet
    cfg = {"patch_size": list(configs.patch_size["11_3d"]), "spacings": list(configs.spacings["11_3d"]), "in_channels": 5, "n_class": 4}
    me = types.SimpleNamespace(args=types.SimpleNamespace(depth=5, min_fmap=4, config_dict=cfg))
    in_ch, n_class, kernels, strides, patch = nn_unet.NNUnet.get_unet_params(me)
    json.dump({"config": cfg, "depth": 5, "min_fmap": 4, "kernels": kernels, "strides": strides, "patch_size": patch,
               "tta_flips": [[2], [3], [4], [2, 3], [2, 4], [3, 4], [2, 3, 4]]},
              open(os.path.join(GOLDEN, "nnunet_unet_params.json"), "w"), indent=0)

    # 4. the command line
    json.dump(parser_flags(os.path.join(args.reference, "utils", "args.py")), open(os.path.join(GOLDEN, "nnunet_cli_flags.json"), "w"), indent=0)
    for f in ("nnunet_unet3d.npz", "nnunet_state_dict.json", "nnunet_unet_params.json", "nnunet_cli_flags.json"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
