"""BERT-Large inference timing: BertPredictor.encode, packed against padded, fp16.

    python tools/bert_infer_perf.py [--reps 7] [--out profiles/bert_infer_perf.json]

Batch sizes 1, 8, 64, 256 at max_seq_length 128 and 384; per point four fixed-seed length sets with mean fill near 1.0, 0.75, 0.5 and
0.25 of max_seq_length (1.0: every sequence full; 0.75: uniform on [S/2, S]; 0.5: uniform on [1, S]; 0.25: uniform on [1, S/2]; the
fill actually drawn is recorded).  The two paths run in ONE process on the same inputs, interleaved (one window of each inside every
repetition, after warm-up calls of both at that shape); a window is a pair of HIP events around `inner` back-to-back encode calls,
host synchronisation of the routing included.  Reported: median / min / max ms per call over the repetitions and the ratio of the
medians, packed / padded.  At fill 1.0 the packed path is forced (the router would not take it): its cost when nothing is saved.
Random weights (timing does not depend on them).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearningexamples_amd.bert.infer import BertPredictor                          # noqa: E402
from deeplearningexamples_amd.bert.model import LARGE, BertForPreTraining              # noqa: E402

BATCHES = (1, 8, 64, 256)
SEQS = (128, 384)
FILLS = {"1.0": (1.0, 1.0), "0.75": (0.5, 1.0), "0.5": (0.0, 1.0), "0.25": (0.0, 0.5)}       # uniform range as fractions of S


def draw_lengths(b, s, lo, hi, g):
    if lo == hi:
        return [s] * b
    return torch.randint(max(1, int(lo * s)), int(hi * s) + 1, (b,), generator=g).tolist()


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def interleaved(legs, inner, reps):
    for fn in legs.values():                                  # warm every leg at this shape (code objects, allocator, workspaces)
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(window(fn, inner))
    return {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bert_infer_perf.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = dict(LARGE)
    predictor = BertPredictor(BertForPreTraining(cfg, device=dev), compute_dtype=torch.float16, device=dev)
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(1)
    rows = []
    for s in SEQS:
        for b in BATCHES:
            for name, (lo, hi) in FILLS.items():
                lengths = draw_lengths(b, s, lo, hi, g)
                ids = torch.randint(0, cfg["real_vocab"], (b, s), generator=g).to(dev)
                mask = (torch.arange(s)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64).to(dev)
                tt = torch.zeros_like(ids)
                legs = {"packed": lambda: predictor.encode(ids, tt, mask, packed=True),
                        "padded": lambda: predictor.encode(ids, tt, mask, packed=False)}
                inner = 10 if b * s <= 8192 else 3
                res = interleaved(legs, inner, a.reps)
                predictor.encode(ids, tt, mask)
                routed = predictor.last_route
                rows.append(dict(max_seq_length=s, batch=b, fill_target=float(name), fill=sum(lengths) / float(b * s),
                                 tokens=sum(lengths), inner=inner, reps=a.reps, default_route=routed, **res,
                                 packed_over_padded=res["packed"]["ms_median"] / res["padded"]["ms_median"]))
                print(json.dumps(rows[-1]), flush=True)
    result = dict(tool="tools/bert_infer_perf.py", device=torch.cuda.get_device_name(0), dtype="fp16", model="BERT-Large (24 x 1024, 16 heads)",
                  call="BertPredictor.encode(layers=(-1,))", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
