"""python -m deeplearningexamples_amd.bert.extract_features -- per-token BERT features of a text file, one JSON object per line.

The flags of LanguageModeling/BERT/extract_features.py (--input_file, --output_file, --do_lower_case, --layers, --max_seq_length,
--batch_size, --no_cuda, --local_rank); its downloading --bert_model is replaced with --vocab_file, --config_file and
--init_checkpoint (as LanguageModeling/BERT/inference.py takes them), and --amp-dtype picks the 16-bit type.  Input lines are
`text` or `text_a ||| text_b`; output lines are
    {"linex_index": i, "features": [{"token": t, "layers": [{"index": l, "values": [...]}]}]}
with the values rounded to 6 places, for the real tokens of line i ([CLS] / [SEP] included, padding left out).  Sentences are not
run as a padded [B, max_seq_length] rectangle: BertPredictor packs each batch's real tokens (bert/infer.py).
"""
import argparse
import collections
import json

import torch

from .tokenization import BertTokenizer, build_input, parse_line


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--input_file", required=True)
    p.add_argument("--output_file", required=True)
    p.add_argument("--vocab_file", required=True, help="one WordPiece token per line")
    p.add_argument("--config_file", required=True, help="bert_config.json")
    p.add_argument("--init_checkpoint", required=True, help="ckpt_<step>.pt (a dictionary with a 'model' key) or a bare state dict")
    p.add_argument("--do_lower_case", action="store_true", help="set for an uncased vocabulary")
    p.add_argument("--layers", default="-1,-2,-3,-4", type=str)
    p.add_argument("--max_seq_length", default=128, type=int,
                   help="longer inputs are truncated; shorter ones are NOT padded on the device")
    p.add_argument("--batch_size", default=32, type=int)
    p.add_argument("--local_rank", type=int, default=-1, help="accepted for command-line compatibility; one GPU is used")
    p.add_argument("--no_cuda", action="store_true", help="there is no CPU path")
    p.add_argument("--amp-dtype", dest="amp_dtype", default="fp16", choices=["fp16", "bf16"])
    args = p.parse_args(argv)
    if args.no_cuda:
        raise SystemExit("--no_cuda: this path runs on the MI355X only")
    try:
        args.layer_indexes = [int(x) for x in args.layers.split(",")]
    except ValueError:
        raise SystemExit("--layers: a comma-separated list of integers (got %r)" % args.layers)
    if args.max_seq_length < 3 or args.batch_size < 1:
        raise SystemExit("--max_seq_length must be at least 3 and --batch_size at least 1")
    return args


def read_inputs(path, tokenizer, seq_length):
    """-> list of (tokens, input_ids, input_mask, token_type_ids), one per line of the file."""
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            a, b = parse_line(line)
            out.append(build_input(tokenizer, a, b, seq_length))
    return out


def feature_record(index, tokens, layer_indexes, layer_values):
    """One output object: layer_values[j] is a [>= len(tokens), H] tensor (any device) of layer layer_indexes[j]."""
    rows = [v[:len(tokens)].float().cpu().tolist() for v in layer_values]
    feats = []
    for i, tok in enumerate(tokens):
        layers = [collections.OrderedDict([("index", l), ("values", [round(x, 6) for x in rows[j][i]])])
                  for j, l in enumerate(layer_indexes)]
        feats.append(collections.OrderedDict([("token", tok), ("layers", layers)]))
    return collections.OrderedDict([("linex_index", index), ("features", feats)])


def write_features(fh, index, tokens, layer_indexes, layer_values):
    fh.write(json.dumps(feature_record(index, tokens, layer_indexes, layer_values)) + "\n")


def main(argv=None):
    args = parse_args(argv)
    from .infer import BertPredictor
    from .model import config_from_json
    cfg = config_from_json(args.config_file)
    dtype = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    ckpt = torch.load(args.init_checkpoint, map_location="cpu", weights_only=False)
    predictor = BertPredictor(ckpt, cfg, compute_dtype=dtype, device="cuda")
    tokenizer = BertTokenizer(args.vocab_file, do_lower_case=args.do_lower_case)
    inputs = read_inputs(args.input_file, tokenizer, args.max_seq_length)
    with open(args.output_file, "w", encoding="utf-8") as out:
        for start in range(0, len(inputs), args.batch_size):
            chunk = inputs[start:start + args.batch_size]
            ids, mask, types = (torch.tensor([c[k] for c in chunk], dtype=torch.int64) for k in (1, 2, 3))
            layers, _ = predictor.encode(ids, types, mask, layers=args.layer_indexes)
            layers = [l.float().cpu() for l in layers]
            for i, c in enumerate(chunk):
                write_features(out, start + i, c[0], args.layer_indexes, [l[i] for l in layers])


if __name__ == "__main__":
    main()
