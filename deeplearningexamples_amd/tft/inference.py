"""Command line of the TFT recipe's inference (the reference's PyTorch/Forecasting/TFT/inference.py):

    python -m deeplearningexamples_amd.tft.inference --checkpoint checkpoint.pt --data test.csv --tgt_scalers tgt_scalers.bin \\
        --cat_encodings cat_encodings.bin --amp [--amp-dtype bf16] [--batch_size 64] [--save_predictions --results DIR]

The flag names and defaults are the reference's (inference.py:223-239) plus --amp / --amp-dtype.  It prints the reference's
`Test q-risk: P10 .. | P50 .. | P90 ..` and latency lines; --save_predictions writes DIR/predictions/<id>/{targets,P10,P50,P90}.csv.
Not built (one-line exits): --visualize and --joint_visualization (matplotlib / tensorboard plots), fp32.
The scalers are whatever the preprocessing pickled: any object with inverse_transform (scikit-learn is needed only if the pickle
holds its classes).
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch

from . import data as D
from .infer import TFTForecaster
from .model import load_checkpoint


def get_parser():
    p = argparse.ArgumentParser(description="TFT inference on the MI355X")
    p.add_argument("--checkpoint", type=str, help="Path to the checkpoint")
    p.add_argument("--data", type=str, help="Path to the test split of the dataset")
    p.add_argument("--tgt_scalers", type=str, help="Path to the tgt_scalers.bin file produced by the preprocessing")
    p.add_argument("--cat_encodings", type=str, help="Path to the cat_encodings.bin file produced by the preprocessing")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--visualize", action="store_true", help="not built: per-example plots")
    p.add_argument("--joint_visualization", action="store_true", help="not built: per-series plots")
    p.add_argument("--save_predictions", action="store_true")
    p.add_argument("--results", type=str, default="/results")
    p.add_argument("--log_file", type=str, default="dllogger.json")
    p.add_argument("--disable_benchmark", action="store_true", help="Disable benchmarking mode")
    p.add_argument("--amp", action="store_true", help="16-bit inference (the only precision built)")
    p.add_argument("--amp-dtype", default=None, choices=["fp16", "bf16"], help="16-bit storage type (--amp = fp16)")
    return p


class _Meter:
    """Wall time per batch; in benchmark mode the device is drained around every lap (the reference's PerformanceMeter)."""

    def __init__(self, sync):
        self.sync, self.intervals, self.total, self.count = sync, [], 0.0, 0
        self.lap()

    def lap(self):
        if self.sync:
            torch.cuda.synchronize()
        self.t0 = time.time()

    def update(self, n, exclude):
        if self.sync:
            torch.cuda.synchronize()
        d = time.time() - self.t0
        self.intervals.append(d)
        if not exclude:
            self.total, self.count = self.total + d, self.count + n
        self.t0 = time.time()

    def p(self, i):
        return sorted(self.intervals)[min(int(len(self.intervals) * i / 100), len(self.intervals) - 1)]


def _write_csv(path, rows):
    with open(path, "w") as f:
        f.write("," + ",".join("t+%d" % (i + 1) for i in range(rows.shape[1])) + "\n")
        for i, r in enumerate(rows):
            f.write("%d," % i + ",".join(repr(float(v)) for v in r) + "\n")


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.visualize or args.joint_visualization:
        raise SystemExit("--visualize / --joint_visualization are not built: use --save_predictions and plot the CSV files")
    if not args.amp and args.amp_dtype is None:
        raise SystemExit("this path computes in 16 bits: pass --amp (or --amp-dtype bf16); the reference's fp32 recipe is not built")
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    config, model = load_checkpoint(args.checkpoint)
    fc = TFTForecaster(model, dtype=dtype)
    dataset = D.TFTDataset(args.data, config)
    with open(args.tgt_scalers, "rb") as f:
        scalers = pickle.load(f)
    n_batches = (len(dataset) + args.batch_size - 1) // args.batch_size
    meter = _Meter(not args.disable_benchmark)
    preds, targets, ids = [], [], []
    for step, batch in enumerate(D.batches(dataset, args.batch_size)):
        meter.lap()
        dev = {k: (v.cuda() if v.numel() else None) for k, v in batch.items() if k != "id"}
        preds.append(fc.forecast(dev))
        ids.append(batch["id"][:, 0, :])
        targets.append(batch["target"][:, config.encoder_length:, :])
        meter.update(args.batch_size, exclude=step in (0, 1, 2, n_batches - 1))
    preds = torch.cat(preds).cpu().numpy()
    targets = torch.cat(targets).numpy()
    ids = torch.cat(ids).numpy().reshape(-1)
    if config.scale_per_id:
        un = lambda v: D.unscale_per_id(v, ids, scalers)
    else:
        un = lambda v: D.unscale(v, scalers[""])
    u_pred = np.stack([un(preds[:, :, i]) for i in range(len(config.quantiles))], axis=-1)
    u_tgt = un(targets[:, :, 0])[:, :, None]
    if args.save_predictions:
        for key in np.unique(ids):
            d = os.path.join(args.results, "predictions", str(int(key)))
            os.makedirs(d, exist_ok=True)
            sel = ids == key
            _write_csv(os.path.join(d, "targets.csv"), u_tgt[sel, :, 0])
            for i, q in enumerate(config.quantiles):
                _write_csv(os.path.join(d, "P%d.csv" % int(q * 100)), u_pred[sel, :, i])
    risk = D.qrisk(u_pred, u_tgt, np.array(config.quantiles))
    print("Test q-risk: P10 {} | P50 {} | P90 {}".format(risk[0].item(), risk[1].item(), risk[2].item()))
    lat = meter.total / max(len(meter.intervals), 1)
    print("Latency:\n\tAverage {:.3f}s\n\tp90 {:.3f}s\n\tp95 {:.3f}s\n\tp99 {:.3f}s".format(lat, meter.p(90), meter.p(95), meter.p(99)))
    return risk


if __name__ == "__main__":
    main(sys.argv[1:])
