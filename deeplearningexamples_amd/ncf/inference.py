"""Command line of the NCF recipe's inference benchmark (the reference's PyTorch/Recommendation/NCF/inference.py):

    python -m deeplearningexamples_amd.ncf.inference --fp16 [--amp-dtype bf16] [--load_checkpoint_path model.pth]
        [--batch_sizes 1,4,...,1048576] [--num_batches 200] [--log_path log.json]

Every flag and default is the reference's (inference.py:28-51) plus --amp-dtype / --graphs / --unfused.  Per batch size it logs
batch_N_mean_throughput, batch_N_mean_latency and the p90 / p95 / p99 latencies of host time around one call + synchronize, the
first 10 calls dropped, as the reference does.  fp32 is not built (one-line exit).
"""
import argparse
import sys
import time

import numpy as np
import torch

from ..utils import dllogger
from .infer import NeuMFScorer
from .model import NeuMFModel


def get_parser():
    p = argparse.ArgumentParser(description="Benchmark inference performance of the NCF model")
    p.add_argument("--load_checkpoint_path", default=None, type=str, help="Path to the checkpoint file to be loaded")
    p.add_argument("--n_users", default=138493, type=int, help="Number of users (default: ml-20m after preprocessing)")
    p.add_argument("--n_items", default=26744, type=int, help="Number of items (default: ml-20m after preprocessing)")
    p.add_argument("-f", "--factors", type=int, default=64, help="Number of predictive factors")
    p.add_argument("--dropout", type=float, default=0.5, help="Dropout probability (evaluation: never applied)")
    p.add_argument("--layers", nargs="+", type=int, default=[256, 256, 128, 64], help="Sizes of hidden layers for MLP")
    p.add_argument("--batch_sizes", default="1,4,16,64,256,1024,4096,16384,65536,262144,1048576", type=str,
                   help="A list of comma-separated batch size values to benchmark")
    p.add_argument("--num_batches", default=200, type=int, help="Number of batches for which to measure latency and throughput")
    p.add_argument("--fp16", action="store_true", default=False, help="16-bit inference (the only precision built)")
    p.add_argument("--log_path", default="log.json", type=str, help="Path for the JSON log")
    p.add_argument("--amp-dtype", default=None, choices=["fp16", "bf16"], help="16-bit storage type (--fp16 = fp16)")
    p.add_argument("--graphs", action="store_true", help="replay one captured graph per batch size")
    p.add_argument("--unfused", action="store_true", help="the gather + GEMM chain instead of the fused kernel")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not args.fp16 and args.amp_dtype is None:
        raise SystemExit("this path computes in 16 bits: pass --fp16 (or --amp-dtype bf16); the reference's fp32 recipe is not built")
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    dllogger.init(backends=[dllogger.JSONStreamBackend(dllogger.Verbosity.VERBOSE, args.log_path),
                            dllogger.StdOutBackend(dllogger.Verbosity.VERBOSE)])
    dllogger.log(data=vars(args), step="PARAMETER")
    model = NeuMFModel(args.n_users, args.n_items, args.factors, args.layers, args.dropout)
    if args.load_checkpoint_path:
        model.load_state_dict(torch.load(args.load_checkpoint_path, map_location="cpu"))
    scorer = NeuMFScorer(model.eval(), dtype=dtype, graphs=args.graphs, fused=not args.unfused)
    batch_sizes = [int(s) for s in args.batch_sizes.split(",")]
    result = {}
    for b in batch_sizes:
        print("benchmarking batch size: ", b)
        users = torch.randint(0, args.n_users, (b,), dtype=torch.int64, device=scorer.dev)
        items = torch.randint(0, args.n_items, (b,), dtype=torch.int64, device=scorer.dev)
        latencies = []
        for i in range(args.num_batches):
            torch.cuda.synchronize()
            t0 = time.time()
            scorer.predict(users, items)
            torch.cuda.synchronize()
            t1 = time.time()
            if i >= 10:                               # warm-up calls
                latencies.append(t1 - t0)
        if not latencies:
            raise SystemExit("--num_batches %d leaves nothing after the 10 warm-up calls" % args.num_batches)
        result["batch_%d_mean_throughput" % b] = b / np.mean(latencies)
        result["batch_%d_mean_latency" % b] = float(np.mean(latencies))
        for q in (90, 95, 99):
            result["batch_%d_p%d_latency" % (b, q)] = float(np.percentile(latencies, q))
    for b in batch_sizes:
        dllogger.metadata("batch_%d_mean_throughput" % b, {"unit": "samples/s"})
        for q in ("mean", "p90", "p95", "p99"):
            dllogger.metadata("batch_%d_%s_latency" % (b, q), {"unit": "s"})
    dllogger.log(data=result, step=tuple())
    dllogger.flush()
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
