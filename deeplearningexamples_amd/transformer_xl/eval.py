"""Transformer-XL evaluation on WikiText-103 checkpoints (LanguageModeling/Transformer-XL/pytorch/eval.py).

    python -m deeplearningexamples_amd.transformer_xl.eval --cuda --fp16 --model checkpoint_best.pt --data wikitext-103 \
        --split test --tgt_len 64 --mem_len 640 --clamp_len 400 --same_length --batch_size 16 [--amp-dtype bf16]
    python -m deeplearningexamples_amd.transformer_xl.eval --cuda --fp16 --model checkpoint_best.pt --manual "some raw text"

The flag names and defaults are the reference's (eval.py:41-151) plus --amp-dtype; every flag parses, --config_file / --config read
the reference's YAML (its `eval` section).  valid.txt / test.txt are encoded with the CHECKPOINT's vocabulary, `<eos>` behind every
line; the dataset cache `cache.pt` (a pickled Corpus) is not read.  The log lines are the reference's; perplexity is over the warm
tokens (LMOrderedIterator prepends ceil(mem_len / tgt_len) warm-up batches so that every scored token sees a full memory).

The running loss stays on the device and is read once per --log_interval; segment latencies are device-event times, resolved at
the same moments.

Not built, one line each before any GPU work: --type torchscript / --save_torchscript / --load_torchscript, --manual_vocab bpe,
datasets other than wt103, fp32 (pass --fp16 or --amp-dtype), --manual_config (a randomly initialised model scores nothing), several
processes, and what model.check_config rejects (attn_type != 0, pre_lnorm, sample_softmax > 0, ext_len > 0, d_head != 64).
"""
import argparse
import json
import logging
import math
import os
import pickle
import re
import sys
import time
import warnings

import numpy as np
import torch


def get_parser(config=None):
    parser = argparse.ArgumentParser(description="Transformer-XL language model evaluation (MI355X)",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--config", default="default")
    parser.add_argument("--config_file", default=None)
    parser.add_argument("--work_dir", default="LM-TFM", type=str, help="experiment directory")
    parser.add_argument("--debug", action="store_true", help="run in debug mode (do not create exp dir)")
    parser.add_argument("--data", type=str, default="../data/wikitext-103", help="location of the data corpus")
    parser.add_argument("--manual", type=str, default=None, nargs="+", help="run model on raw input data")
    parser.add_argument("--dataset", type=str, default="wt103", choices=["wt103", "lm1b", "enwik8", "text8"], help="dataset name")
    parser.add_argument("--split", type=str, default="all", choices=["all", "valid", "test"], help="which split to evaluate")
    parser.add_argument("--affinity", type=str, default="single_unique",
                        choices=["socket", "single", "single_unique", "socket_unique_interleaved", "socket_unique_continuous",
                                 "disabled"], help="type of CPU affinity (accepted, not applied)")
    parser.add_argument("--type", type=str, default="pytorch", choices=["pytorch", "torchscript"], help="type of runtime to use")
    parser.add_argument("--batch_size", type=int, default=16, help="batch size")
    parser.add_argument("--tgt_len", type=int, default=64, help="number of tokens to predict")
    parser.add_argument("--ext_len", type=int, default=0, help="length of the extended context")
    parser.add_argument("--mem_len", type=int, default=640, help="length of the retained previous heads")
    parser.add_argument("--seed", type=int, default=1111, help="Random seed")
    parser.add_argument("--clamp_len", type=int, default=-1, help="max positional embedding index")
    parser.add_argument("--cuda", action="store_true", help="Run evaluation on the GPU (the only path there is)")
    parser.add_argument("--model", type=str, default="", help="path to the checkpoint")
    parser.add_argument("--manual_config", type=json.loads, default=None, help="Manually specify config for the model")
    parser.add_argument("--manual_vocab", type=str, default="word", choices=["word", "bpe"], help="Manually specify type of vocabulary")
    parser.add_argument("--fp16", action="store_true", help="Run in fp16")
    parser.add_argument("--amp-dtype", default=None, choices=["fp16", "bf16"], help="16-bit storage type (--fp16 = fp16)")
    parser.add_argument("--log_all_ranks", action="store_true", help="Enable logging for all distributed ranks")
    parser.add_argument("--dllog_file", type=str, default="eval_log.json", help="Name of the DLLogger output file")
    parser.add_argument("--same_length", action="store_true", help="set same length attention with masking")
    parser.add_argument("--no_env", action="store_true", help="Do not print info on execution env")
    parser.add_argument("--log_interval", type=int, default=10, help="Report interval")
    parser.add_argument("--target_perplexity", type=float, default=None, help="target perplexity")
    parser.add_argument("--target_throughput", type=float, default=None, help="target throughput")
    parser.add_argument("--save_data", action="store_true", help="save latency and throughput data to a file")
    parser.add_argument("--repeat", type=int, default=1, help="loop over the dataset REPEAT times")
    parser.add_argument("--max_size", type=int, default=None, help="run inference on up to MAX_SIZE batches")
    parser.add_argument("--percentiles", nargs="+", default=[90, 95, 99], help="percentiles for latency confidence intervals")
    parser.add_argument("--save_torchscript", default=None, type=str, help="save torchscript model to a file")
    parser.add_argument("--load_torchscript", default=None, type=str, help="load torchscript model from a file")
    parser.add_argument("--local_rank", type=int, default=os.getenv("LOCAL_RANK", 0), help="Used for multi-process training.")
    if config:
        parser.set_defaults(**config)
    return parser


def load_yaml_section(config_file, config):
    """eval.py:56-60: the `eval` section of entry `config` of the reference's YAML (anchors and merge keys included)."""
    from ..utils.state import load_config
    doc = load_config(config_file)
    if config not in doc or "eval" not in (doc[config] or {}):
        raise SystemExit("--config %s: %s has no such entry with an `eval` section" % (config, config_file))
    out = dict(doc[config]["eval"])
    if isinstance(out.get("manual_config"), str):
        out["manual_config"] = json.loads(out["manual_config"])
    return out


def parse_args(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--config", default="default")
    pre.add_argument("--config_file", default=None)
    cfg_args, _ = pre.parse_known_args(argv)
    config = load_yaml_section(cfg_args.config_file, cfg_args.config) if (cfg_args.config is not None and cfg_args.config_file) else {}
    args, _ = get_parser(config).parse_known_args(argv)
    if args.manual:
        args.batch_size = 1
    if args.same_length and args.tgt_len > args.mem_len:
        warnings.warn("--same_length is intended to be used with large mem_len relative to tgt_len")
    if args.ext_len < 0:
        raise SystemExit("Extended context length must be non-negative")
    reject(args)
    return args


def reject(args):
    """What this package does not build: one line each, before any GPU work."""
    if args.type != "pytorch":
        raise SystemExit("--type torchscript: TorchScript is not built")
    if args.save_torchscript or args.load_torchscript:
        raise SystemExit("--save_torchscript / --load_torchscript: TorchScript is not built")
    if args.manual_vocab == "bpe":
        raise SystemExit("--manual_vocab bpe: the GPT-2 vocabulary is not built; word vocabularies only")
    if args.dataset != "wt103":
        raise SystemExit("--dataset %s: only wt103 is built" % args.dataset)
    if args.ext_len > 0:
        raise SystemExit("--ext_len %d: an extended context is not built" % args.ext_len)
    if not args.fp16 and args.amp_dtype is None:
        raise SystemExit("this path computes in 16 bits: pass --fp16 (or --amp-dtype bf16); the reference's fp32 recipe is not built")
    if args.manual_config is not None:
        raise SystemExit("--manual_config: a randomly initialised model scores nothing; pass --model CHECKPOINT")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("WORLD_SIZE > 1: evaluation on several GPUs is not built")
    if not args.manual and args.split not in ("valid", "test"):
        raise SystemExit("Unknown split")                                    # eval.py:372-373: `all` is its default and is refused


class LMOrderedIterator:
    """data_utils.py:29-116 for evaluation on one process: the stream cut into `bsz` columns, `bptt` rows per batch, and with a
    memory ceil(mem_len / bptt) warm-up batches in front, taken from the END of every column's left neighbour (`roll`), which are
    scored but not counted (`warm` False).  Yields HOST tensors."""

    def __init__(self, data, bsz, bptt, mem_len=None, ext_len=None, warmup=True):
        self.bsz, self.bptt, self.ext_len, self.mem_len, self.warmup = bsz, bptt, ext_len if ext_len is not None else 0, mem_len, warmup
        n_step = data.size(0) // bsz
        if n_step < 2:
            raise ValueError("the stream holds %d tokens: fewer than 2 per column of a batch of %d" % (data.size(0), bsz))
        self.data = data[:n_step * bsz].view(bsz, -1).t().contiguous()
        if mem_len and warmup:
            self.warmup_batches = (mem_len + bptt - 1) // bptt
            self.warmup_elems = self.warmup_batches * bptt
            warmup_data = self.data.roll((self.warmup_elems, 1), (0, 1))[:self.warmup_elems]
            self.data = torch.cat((warmup_data, self.data))
        self.n_batch = (self.data.size(0) + self.bptt - 1) // self.bptt

    def get_batch(self, i):
        seq_len = min(self.bptt, self.data.size(0) - 1 - i)
        beg = max(0, i - self.ext_len)
        data, target = self.data[beg:i + seq_len], self.data[i + 1:i + 1 + seq_len]
        warm = i >= self.warmup_elems if (self.mem_len and self.warmup) else True
        return data, target, seq_len, warm

    def __iter__(self):
        for i in range(0, self.data.size(0) - 1, self.bptt):
            yield self.get_batch(i)


def tokenize_raw(text):
    """data_utils.py:330-338.  The reference runs the Moses tokenizer first; where `sacremoses` is not installed the text is split
    on white space only, and the WikiText conventions ( @.@  @,@  @-@ ) are applied either way."""
    try:
        import sacremoses
        text = sacremoses.MosesTokenizer("en").tokenize(text, return_str=True)
    except ImportError:
        text = " ".join(text.split())
    text = re.sub(r"&quot;", '"', text)
    text = re.sub(r"&apos;", "'", text)
    text = re.sub(r"(\d)\.(\d)", r"\1 @.@ \2", text)
    text = re.sub(r"(\d),(\d)", r"\1 @,@ \2", text)
    text = re.sub(r"(\w)-(\w)", r"\1 @-@ \2", text)
    return text


def format_log(loss, split, args):
    if args.dataset in ["enwik8", "text8"]:
        return "| {0} loss {1:5.2f} | {0} bpc {2:9.5f} ".format(split, loss, loss / math.log(2))
    return "| {0} loss {1:5.2f} | {0} ppl {2:9.3f} ".format(split, loss, math.exp(loss))


class AverageMeter:
    """utils/exp_utils.py:30-56."""

    def __init__(self, warmup=0, keep=False):
        self.warmup, self.keep = warmup, keep
        self.val = self.avg = self.sum = self.count = self.iters = 0
        self.vals = []

    def update(self, val, n=1):
        self.iters += 1
        self.val = val
        if self.iters > self.warmup:
            self.sum += val * n
            self.count += n
            self.avg = self.sum / self.count
            if self.keep:
                self.vals.append(val)


def benchmark(test_perplexity=None, target_perplexity=None, test_throughput=None, target_throughput=None):
    """utils/exp_utils.py:103-125."""
    def test(achieved, target, name, higher_better=True):
        if target is None or achieved is None:
            return True
        logging.info("%s achieved: %.2f target: %.2f" % (name, achieved, target))
        ok = achieved >= target if higher_better else achieved <= target
        logging.info("%s test %s" % (name, "passed" if ok else "failed"))
        return ok
    passed = test(test_perplexity, target_perplexity, "Perplexity", False)
    return test(test_throughput, target_throughput, "Throughput") and passed


def evaluate(eval_iter, evaluator, meters, log_interval, max_size=None, repeat=1):
    """eval.py:171-253.  The per-segment loss and the warm sum stay on the device; they, and the event times of the segments since
    the last report, are read once per `log_interval` segments and once at the end."""
    dev = evaluator.dev
    total_len, eval_step, idx = 0, 0, -1
    total_loss = torch.zeros((), dtype=torch.float64, device=dev)
    log_loss = torch.zeros((), dtype=torch.float32, device=dev)
    pending = []                                                  # (start event, end event, target tokens) not yet resolved
    log_throughput = log_latency = 0.0
    start_time = time.time()

    def resolve():
        nonlocal log_throughput, log_latency
        torch.cuda.synchronize(dev)
        for s, e, ntok in pending:
            elapsed = s.elapsed_time(e) / 1000.0
            meters["eval_latency"].update(elapsed)
            meters["eval_throughput"].update(ntok / elapsed, elapsed)
            log_latency += elapsed
            log_throughput += ntok / elapsed
        del pending[:]

    evaluator.reset()
    for _ in range(repeat):
        for idx, (data, target, seq_len, warm) in enumerate(eval_iter):
            if max_size and idx >= max_size:
                break
            eval_step += 1
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            loss = evaluator.segment(data, target).mean()
            e.record()
            pending.append((s, e, target.numel()))
            log_loss += loss
            if warm:
                total_loss += seq_len * loss.double()
                total_len += seq_len
            if eval_step % log_interval == 0:
                resolve()
                ll = float(log_loss.item()) / log_interval            # the interval's one read of the loss
                log_loss.zero_()
                logging.info("| step {:>8d} | batches {:>6d} / {:d} | ms/batch {:5.2f} | tok/s {:7.0f} | loss {:5.2f} | ppl {:5.2f}".format(
                    eval_step, idx + 1, eval_iter.n_batch, log_latency / log_interval * 1000, log_throughput / log_interval, ll,
                    math.exp(ll)))
                log_throughput = log_latency = 0.0
    resolve()
    total_time = time.time() - start_time
    logging.info("Time : {:.2f}s, {:.2f}ms/segment".format(total_time, 1000 * total_time / (idx + 1)))
    if total_len == 0:
        raise SystemExit("no warm tokens were scored: the stream is shorter than its warm-up")
    return float(total_loss.item()) / total_len


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout, force=True)
    from .infer import TransformerXLEvaluator
    from .model import Vocab, check_config, load_checkpoint

    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.model:
        model_path = args.model
    elif args.work_dir:
        model_path = os.path.join(args.work_dir, "checkpoint_best.pt")
    else:
        raise SystemExit("Specify path to checkpoint using --model or --work_dir")
    if not os.path.exists(model_path):
        raise SystemExit("%s: no such checkpoint" % model_path)
    logging.info("Loading checkpoint from %s" % model_path)
    ckpt = load_checkpoint(model_path)
    vocab = ckpt.get("vocab")
    ck_args = ckpt.get("args")
    if getattr(ck_args, "vocab", "word") != "word" or not isinstance(vocab, Vocab):
        raise SystemExit("the checkpoint was trained with a %r vocabulary: word vocabularies only" % getattr(ck_args, "vocab", None))
    cfg = dict(ckpt["model_config"], tgt_len=args.tgt_len, ext_len=args.ext_len, mem_len=args.mem_len, clamp_len=args.clamp_len,
               same_length=args.same_length)
    try:
        check_config(cfg)                                                        # before any GPU work
    except ValueError as e:
        raise SystemExit(str(e))

    if args.manual:
        symbols = vocab.tokenize(tokenize_raw(" ".join(args.manual)), add_eos=True)
        tensor = vocab.convert_to_tensor(symbols)
        it = LMOrderedIterator(tensor, bsz=args.batch_size, bptt=args.tgt_len, ext_len=args.ext_len, warmup=False)
    else:
        path = os.path.join(args.data, "%s.txt" % args.split)
        if not os.path.exists(path):
            raise SystemExit("%s: no such file (the corpus is read as text; cache.pt is not)" % path)
        tensor = vocab.encode_file(path, ordered=True, add_eos=True)
        it = LMOrderedIterator(tensor, bsz=args.batch_size, bptt=args.tgt_len, mem_len=args.mem_len, ext_len=args.ext_len)

    if not args.cuda or not torch.cuda.is_available():
        raise SystemExit("evaluation runs on the GPU only: pass --cuda on a machine that has one (there is no CPU path)")
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    math_str = "bf16" if dtype == torch.bfloat16 else "fp16"
    evaluator = TransformerXLEvaluator.from_checkpoint(ckpt, args.batch_size, args.tgt_len, args.mem_len, clamp_len=args.clamp_len,
                                                       same_length=args.same_length, dtype=dtype)
    logging.info("Evaluating with: math %s type %s bsz %d tgt_len %d ext_len %d mem_len %d clamp_len %d" % (
        math_str, args.type, args.batch_size, args.tgt_len, args.ext_len, args.mem_len, args.clamp_len))
    warmup = args.mem_len // args.tgt_len + 2
    meters = {"eval_throughput": AverageMeter(warmup=warmup, keep=args.save_data),
              "eval_latency": AverageMeter(warmup=warmup, keep=args.save_data)}
    loss = evaluate(it, evaluator, meters, args.log_interval, args.max_size, args.repeat)
    perplexity = math.exp(loss)
    logging.info("=" * 100)
    logging.info(format_log(loss, args.split, args))
    logging.info("=" * 100)
    if args.save_data:
        latency, throughput = np.array(meters["eval_latency"].vals), np.array(meters["eval_throughput"].vals)
        if not args.debug:
            os.makedirs(args.work_dir, exist_ok=True)
            with open(os.path.join(args.work_dir, "eval_data_%d_%s_%s" % (args.batch_size, math_str, args.type)), "wb") as f:
                pickle.dump({"args": args, "throughput": throughput, "latency": latency}, f)
        logging.info("Throughput Avg: %.2f tok/s" % meters["eval_throughput"].avg)
        if latency.size:
            logging.info("Latency Avg: %.2f ms" % (1000.0 * latency.mean()))
            for p in args.percentiles:
                logging.info("Latency %s%%: %.2f ms" % (p, 1000.0 * np.percentile(latency, float(p))))
        logging.info("=" * 100)
    if not benchmark(target_perplexity=args.target_perplexity, test_perplexity=perplexity,
                     target_throughput=args.target_throughput, test_throughput=meters["eval_throughput"].avg):
        sys.exit(1)
    return loss


if __name__ == "__main__":
    main()
