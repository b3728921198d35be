"""The reference's command line (PyTorch/Segmentation/nnUNet/main.py, utils/args.py) for what is built: the BraTS22 UNet3D,

    python -m deeplearningexamples_amd.nnunet.main --exec_mode predict --brats --brats22_model --amp --data DIR --ckpt_path F.ckpt \
        --results OUT [--save_preds] [--tta] [--overlap 0.5] [--blend gaussian] [--benchmark --val_batch_size 2 --test_batches 20]
    python -m deeplearningexamples_amd.nnunet.main --exec_mode evaluate --brats --brats22_model --amp --data DIR --ckpt_path F.ckpt

Every flag of utils/args.py parses.  --data names the preprocessed directory; left at its default /data it means /data/<task>_3d
(and its test/ subdirectory for a prediction run), with config.pkl in /data/<task>_3d, as in the reference.  Training, --dim 2 and any run without --brats22_model (MONAI's DynUNet) exit with one line.
Extra flags of this project: --bf16 (bfloat16 instead of fp16) and --graphs (replay the patch as a captured graph).
"""
import json
import os
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser, ArgumentTypeError, Namespace

import numpy as np
import torch

from . import data as D
from . import model as M
from .metrics import Dice


def _checked(convert, accept, what):
    """An argparse type: `convert` the string, then `accept` the value or report `what` was expected."""
    def parse(text):
        try:
            number = convert(text)
        except ValueError:
            raise ArgumentTypeError("%r is not %s" % (text, what))
        if not accept(number):
            raise ArgumentTypeError("%r is not %s" % (text, what))
        return number
    return parse


# the three value checks of the reference's parser, under its names (the flag table is pinned by name)
positive_int = _checked(int, lambda n: n > 0, "a positive integer")
positive_int.__name__ = "positive_int"
non_negative_int = _checked(int, lambda n: n >= 0, "a non-negative integer")
non_negative_int.__name__ = "non_negative_int"
float_0_1 = _checked(float, lambda x: 0.0 <= x <= 1.0, "a number between 0 and 1")
float_0_1.__name__ = "float_0_1"


# (flag, type, default, choices, nargs) of utils/args.py:40-146, in its order; type None = store_true
FLAGS = (
    ("exec_mode", str, "train", ["train", "evaluate", "predict"], None), ("data", str, "/data", None, None),
    ("results", str, "/results", None, None), ("config", str, None, None, None), ("logname", str, "logs.json", None, None),
    ("task", str, "01", None, None), ("gpus", non_negative_int, 1, None, None), ("nodes", non_negative_int, 1, None, None),
    ("learning_rate", float, 0.0008, None, None), ("gradient_clip_val", float, 0, None, None), ("negative_slope", float, 0.01, None, None),
    ("tta", None, False, None, None), ("brats", None, False, None, None), ("deep_supervision", None, False, None, None),
    ("invert_resampled_y", None, False, None, None), ("amp", None, False, None, None), ("benchmark", None, False, None, None),
    ("focal", None, False, None, None), ("save_ckpt", None, False, None, None), ("nfolds", positive_int, 5, None, None),
    ("seed", non_negative_int, None, None, None), ("skip_first_n_eval", non_negative_int, 0, None, None), ("ckpt_path", str, None, None, None),
    ("ckpt_store_dir", str, "/results", None, None), ("fold", non_negative_int, 0, None, None), ("patience", positive_int, 100, None, None),
    ("batch_size", positive_int, 2, None, None), ("val_batch_size", positive_int, 4, None, None), ("momentum", float, 0.99, None, None),
    ("weight_decay", float, 0.0001, None, None), ("save_preds", None, False, None, None), ("dim", int, 3, [2, 3], None),
    ("resume_training", None, False, None, None), ("num_workers", non_negative_int, 8, None, None), ("epochs", non_negative_int, 1000, None, None),
    ("warmup", non_negative_int, 5, None, None), ("nvol", positive_int, 4, None, None), ("depth", non_negative_int, 5, None, None),
    ("min_fmap", non_negative_int, 4, None, None), ("deep_supr_num", non_negative_int, 2, None, None), ("res_block", None, False, None, None),
    ("filters", int, None, None, "+"), ("layout", str, "NCDHW", None, None), ("brats22_model", None, False, None, None),
    ("norm", str, "instance", ["instance", "instance_nvfuser", "batch", "group"], None), ("data2d_dim", int, 3, [2, 3], None),
    ("oversampling", float_0_1, 0.4, None, None), ("overlap", float_0_1, 0.25, None, None), ("scheduler", None, False, None, None),
    ("optimizer", str, "adam", ["sgd", "adam"], None), ("blend", str, "constant", ["gaussian", "constant"], None),
    ("train_batches", non_negative_int, 0, None, None), ("test_batches", non_negative_int, 0, None, None),
)


def flag_table():
    """name -> {"default", "choices", "store_true", "nargs"}: what tests pin against the reference's parser."""
    return {n: {"default": d, "choices": c, "store_true": t is None, "nargs": na} for n, t, d, c, na in FLAGS}


def get_parser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, prog="deeplearningexamples_amd.nnunet.main")
    for name, typ, default, choices, nargs in FLAGS:
        if typ is None:
            parser.add_argument("--" + name, action="store_true")
        else:
            kw = {"type": typ, "default": default}
            if choices is not None:
                kw["choices"] = choices
            if nargs is not None:
                kw["nargs"] = nargs
            parser.add_argument("--" + name, **kw)
    parser.add_argument("--bf16", action="store_true", help="bfloat16 activations and weights instead of float16")
    parser.add_argument("--graphs", action="store_true", help="replay each patch shape as a captured graph")
    return parser


def get_main_args(argv=None):
    args = get_parser().parse_args(argv)
    if args.config is not None:
        merged = vars(args)
        merged.update(json.load(open(args.config, "r")))
        args = Namespace(**merged)
    return args


def reject(args):
    """One line for everything that is not built; None when the run is in scope."""
    if args.exec_mode == "train" or args.resume_training:
        return "nnU-Net: training is not built (--exec_mode predict or evaluate)"
    if args.dim != 3:
        return "nnU-Net: --dim 2 is not built (the BraTS22 UNet3D is volumetric)"
    if not args.brats22_model:
        return "nnU-Net: only the BraTS22 UNet3D is built: pass --brats22_model (MONAI's DynUNet is not part of the reference's text)"
    if not args.brats:
        return "nnU-Net: --brats22_model has three sigmoid outputs: pass --brats"
    if not args.amp and not args.bf16:
        return "nnU-Net: this path computes in 16 bits: pass --amp (the reference's fp32 / TF32 recipe is not built)"
    if args.gpus != 1 or args.nodes != 1:
        return "nnU-Net: one GPU, one node (the reference's multi-GPU evaluation is not built)"
    if args.invert_resampled_y:
        return "nnU-Net: --invert_resampled_y is not built (BraTS data is not resampled)"
    if args.filters is not None or args.res_block or args.norm != "instance":
        return "nnU-Net: --filters, --res_block and --norm configure MONAI's DynUNet, which is not built"
    if args.ckpt_path is None:
        return "nnU-Net: pass --ckpt_path (a checkpoint of the reference)"
    return None


def build_segmenter(args, config):
    from .infer import BratsSegmenter
    kernels, strides = M.get_unet_params(config["patch_size"], config["spacings"], depth=args.depth, min_fmap=args.min_fmap)
    levels = M.check_envelope(kernels, strides, args.dim)
    if config.get("in_channels", M.IN_CHANNELS) != M.IN_CHANNELS:
        raise M.NNUnetConfigError("nnU-Net: the data has %s input channels, the BraTS22 UNet3D takes %d" % (config.get("in_channels"), M.IN_CHANNELS))
    state, _ = M.load_checkpoint(args.ckpt_path)
    if M.levels_of(state) != levels:
        raise M.NNUnetConfigError("nnU-Net: the checkpoint has %d levels, the data's config asks for %d" % (M.levels_of(state), levels))
    return BratsSegmenter(state, torch.bfloat16 if args.bf16 else torch.float16, graphs=args.graphs, patch_size=config["patch_size"],
                          val_batch_size=args.val_batch_size)


def crop_back(pred, meta):
    """What test_step does with a prediction before it is saved (nn_unet.py:118-135, --brats): the logits [3, d, h, w] are put back
    into the box they were cropped from -- rows 0 and 1 of meta are the box's corners, row 2 the original shape, row 3 the cropped
    shape -- inside a volume of zeros, and the logistic function is taken of all of it (0.5 outside the box)."""
    meta = np.asarray(meta)
    if tuple(int(e) for e in meta[3]) != tuple(pred.shape[1:]):
        raise M.NNUnetConfigError("nnU-Net: prediction %s differs from the cropped shape %s: resampled data is not built" % (tuple(pred.shape[1:]), tuple(meta[3])))
    volume = np.zeros((pred.shape[0],) + tuple(int(e) for e in meta[2]))
    box = tuple(slice(int(lo), int(hi)) for lo, hi in zip(meta[0], meta[1]))
    volume[(slice(None),) + box] = pred
    return 1.0 / (1.0 + np.exp(-volume))


def performance_stats(stamps, batch, mode):
    """The records of the reference's benchmark callback (utils/logger.py:85-99) from one time stamp per batch: images per second
    over the mean interval, the mean interval and its 90th / 95th / 99th percentiles in ms, three decimals."""
    ms = 1000.0 * np.diff(np.asarray(stamps, dtype=np.float64))
    out = {"throughput_" + mode: round(float(1000.0 * batch / ms.mean()), 3), "latency_%s_mean" % mode: round(float(ms.mean()), 3)}
    out.update({"latency_%s_%d" % (mode, q): round(float(np.percentile(ms, q)), 3) for q in (90, 95, 99)})
    return out


def run_benchmark(args, seg, config, data_dir):
    """main.py:100-108 with test_step's benchmark branch: the model on centre crops of the training fold, one warm-up pass and one
    timed pass of --test_batches batches (all of the fold when 0)."""
    (imgs, _), _ = D.fold_files(data_dir, args.nfolds, args.fold)
    bs = args.val_batch_size
    n_batches = len(imgs) // bs if args.test_batches == 0 else args.test_batches
    if n_batches < 2:
        raise M.NNUnetConfigError("nnU-Net: the benchmark needs at least two batches of %d (found %d images)" % (bs, len(imgs)))
    crops = [D.center_crop_pad(np.load(f), config["patch_size"]) for f in imgs[:max(bs, min(len(imgs), 4 * bs))]]
    batches = [torch.from_numpy(np.stack([crops[(b * bs + i) % len(crops)] for i in range(bs)])).to(seg.dev, torch.float32) for b in range(min(n_batches, 4))]
    for timed in (False, True):
        stamps = []
        for b in range(n_batches):
            seg.logits_patch(batches[b % len(batches)])
            if timed:
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
    stats = performance_stats(stamps, bs, args.exec_mode)
    for k, v in stats.items():
        print("DLL - %s : %s" % (k, v))
    with open(os.path.join(args.results, args.logname if args.logname is not None else "perf.json"), "a") as f:
        f.write(json.dumps({"type": "LOG", "step": [], "data": stats}) + "\n")
    return stats


def run_predict(args, seg, data_dir):
    imgs, metas = D.test_files(data_dir, args.exec_mode, args.nfolds, args.fold)
    if not imgs:
        raise FileNotFoundError("No data found in %s with pattern *_x.npy" % data_dir)
    save_dir = None
    if args.save_preds:
        ckpt_name = "_".join(args.ckpt_path.split("/")[-1].split(".")[:-1])
        save_dir = os.path.join(args.results, "predictions_%s_task=%s_fold=%d%s" % (ckpt_name, args.task, args.fold, "_tta" if args.tta else ""))
        os.makedirs(save_dir, exist_ok=True)
        if len(metas) != len(imgs):
            raise FileNotFoundError("nnU-Net: --save_preds needs one *_meta.npy per *_x.npy in %s" % data_dir)
    limit = len(imgs) if args.test_batches == 0 else min(args.test_batches, len(imgs))
    for i in range(limit):
        vol = torch.from_numpy(np.load(imgs[i])).to(seg.dev, torch.float32)
        pred = seg.segment(vol, overlap=args.overlap, blend=args.blend, tta=args.tta).cpu().numpy()
        if save_dir is not None:
            final = crop_back(pred.astype(np.float64), np.load(metas[i]))
            np.save(os.path.join(save_dir, os.path.basename(imgs[i]).replace("_x", "")), final, allow_pickle=False)
    print("nnU-Net: %d volumes predicted%s" % (limit, "" if save_dir is None else ", saved to " + save_dir))


def run_evaluate(args, seg, data_dir):
    _, (imgs, lbls) = D.fold_files(data_dir, args.nfolds, args.fold)
    limit = len(imgs) if args.test_batches == 0 else min(args.test_batches, len(imgs))
    dice = Dice(M.N_CLASS)
    for i in range(limit):
        vol = torch.from_numpy(np.load(imgs[i])).to(seg.dev, torch.float32)
        lbl = torch.from_numpy(np.load(lbls[i]).astype(np.int64)).to(seg.dev)
        pred = seg.segment(vol, overlap=args.overlap, blend=args.blend, tta=args.tta)
        dice.update(pred[None], lbl.reshape((1,) + tuple(pred.shape[1:])))
    d = dice.compute()
    metrics = {"Dice": round(float(d.mean()), 2)}
    metrics.update({"D%d" % (i + 1): round(float(m), 2) for i, m in enumerate(d)})
    print("DLL - " + json.dumps(metrics))
    return metrics


def main(argv=None):
    args = get_main_args(argv)
    why = reject(args)
    if why is not None:
        sys.exit(why)
    try:
        data_dir, config_dir = D.data_paths(args.data, args.task, args.dim, args.exec_mode, args.benchmark)
        config = D.load_config(config_dir)
        seg = build_segmenter(args, config)
        os.makedirs(args.results, exist_ok=True)
        if args.benchmark:
            run_benchmark(args, seg, config, data_dir)
        elif args.exec_mode == "predict":
            run_predict(args, seg, data_dir)
        else:
            run_evaluate(args, seg, data_dir)
    except (M.NNUnetConfigError, FileNotFoundError) as e:
        sys.exit(str(e))


if __name__ == "__main__":
    main()
