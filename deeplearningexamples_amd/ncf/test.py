"""Command line of the NCF recipe's evaluation: the reference's PyTorch/Recommendation/NCF/ncf.py restricted to --mode test.

    python -m deeplearningexamples_amd.ncf.test --data DIR --mode test --load_checkpoint_path model.pth --amp [--amp-dtype bf16]

Every flag of ncf.py parses with its default (ncf.py:55-105), so a command line of the reference carries over; the training flags
are accepted and unused.  --mode train (the reference's default) exits with one line: NeuMF scoring, the test loader and HR@K /
NDCG@K evaluation are what is built.  It logs best_eval_throughput, hr@10 and validation_loss as the reference's test mode does.
--amp (or --amp-dtype) selects the 16-bit type; fp32 is not built.  WORLD_SIZE above 1 exits with one line.
"""
import argparse
import os
import sys
import time

import torch

from ..utils import dllogger
from . import data as D
from .evaluate import evaluate
from .infer import NeuMFScorer
from .model import NeuMFModel


def get_parser():
    p = argparse.ArgumentParser(description="Evaluate a Neural Collaborative Filtering model")
    p.add_argument("--data", type=str, help="Path to the directory containing the feature specification yaml")
    p.add_argument("--feature_spec_file", type=str, default="feature_spec.yaml",
                   help="Name of the feature specification file or path relative to the data directory.")
    p.add_argument("-e", "--epochs", type=int, default=30, help="(training: not built)")
    p.add_argument("-b", "--batch_size", type=int, default=2 ** 20, help="(training: not built)")
    p.add_argument("--valid_batch_size", type=int, default=2 ** 20, help="Number of examples in each validation chunk")
    p.add_argument("-f", "--factors", type=int, default=64, help="Number of predictive factors")
    p.add_argument("--layers", nargs="+", type=int, default=[256, 256, 128, 64], help="Sizes of hidden layers for MLP")
    p.add_argument("-n", "--negative_samples", type=int, default=4, help="(training: not built)")
    p.add_argument("-l", "--learning_rate", type=float, default=0.0045, help="(training: not built)")
    p.add_argument("-k", "--topk", type=int, default=10, help="Rank for test examples to be considered a hit")
    p.add_argument("--seed", "-s", type=int, default=None, help="Manually set random seed for torch")
    p.add_argument("--threshold", "-t", type=float, default=1.0, help="(training: not built)")
    p.add_argument("--beta1", "-b1", type=float, default=0.25, help="(training: not built)")
    p.add_argument("--beta2", "-b2", type=float, default=0.5, help="(training: not built)")
    p.add_argument("--eps", type=float, default=1e-8, help="(training: not built)")
    p.add_argument("--dropout", type=float, default=0.5, help="Dropout probability (evaluation: never applied)")
    p.add_argument("--checkpoint_dir", default="", type=str, help="(training: not built)")
    p.add_argument("--load_checkpoint_path", default=None, type=str, help="Path to the checkpoint file to be loaded before evaluation")
    p.add_argument("--mode", choices=["train", "test"], default="train", type=str, help='Only "test" is built: a single evaluation')
    p.add_argument("--grads_accumulated", default=1, type=int, help="(training: not built)")
    p.add_argument("--amp", action="store_true", help="16-bit evaluation (the only precision built)")
    p.add_argument("--log_path", default="log.json", type=str, help="Path for the JSON log")
    p.add_argument("--amp-dtype", default=None, choices=["fp16", "bf16"], help="16-bit storage type (--amp = fp16)")
    p.add_argument("--graphs", action="store_true", help="replay one captured graph per batch size")
    p.add_argument("--unfused", action="store_true", help="the gather + GEMM chain instead of the fused kernel")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.mode != "test":
        raise SystemExit("--mode train is not built: NeuMF scoring, the test loader and HR@K / NDCG@K evaluation are (pass --mode test)")
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        raise SystemExit("distributed evaluation is not built: run with WORLD_SIZE unset or 1 (got %d)" % world)
    if not args.amp and args.amp_dtype is None:
        raise SystemExit("this path computes in 16 bits: pass --amp (or --amp-dtype bf16); the reference's fp32 recipe is not built")
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    dllogger.init(backends=[dllogger.JSONStreamBackend(dllogger.Verbosity.VERBOSE, args.log_path),
                            dllogger.StdOutBackend(dllogger.Verbosity.VERBOSE)])
    dllogger.metadata("best_eval_throughput", {"unit": "samples/s"})
    dllogger.metadata("hr@10", {"name": "hr@10", "unit": None, "format": ":.5f"})
    dllogger.metadata("validation_loss", {"name": "validation_loss", "unit": None, "format": ":.5f"})
    dllogger.log(data=vars(args), step="PARAMETER")
    if args.seed is not None:
        torch.manual_seed(args.seed)
    spec = D.FeatureSpec.from_yaml(os.path.join(args.data, args.feature_spec_file))
    model = NeuMFModel(spec.cardinality(D.USER_CHANNEL), spec.cardinality(D.ITEM_CHANNEL), args.factors, args.layers, args.dropout)
    if args.load_checkpoint_path:
        model.load_state_dict(torch.load(args.load_checkpoint_path, map_location="cpu"))
    scorer = NeuMFScorer(model.eval(), dtype=dtype, graphs=args.graphs, fused=not args.unfused)
    loader = D.TestLoader(spec, D.load_features(spec, "test"), args.valid_batch_size, world).to(scorer.dev)
    torch.cuda.synchronize()
    t0 = time.time()
    hr, ndcg, loss = evaluate(scorer, loader, args.topk)
    torch.cuda.synchronize()
    dt = time.time() - t0
    dllogger.log(step=tuple(), data={"best_eval_throughput": loader.raw_length / dt, "hr@10": hr, "validation_loss": loss})
    dllogger.flush()
    return hr, ndcg, loss


if __name__ == "__main__":
    main(sys.argv[1:])
