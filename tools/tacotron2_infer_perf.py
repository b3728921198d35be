"""Tacotron2 inference timing in the recipe of the reference's inference_perf.py: a seeded model at the default widths, 128 input
symbols, batches of 1, 4 and 8, fp16 and bf16, a fixed number of decoder steps (early_stopping=False).

    python tools/tacotron2_infer_perf.py [--steps 256] [--reps 7] [--out profiles/tacotron2_infer.json]

Reports, per configuration, the event-timed decoder loop (ms per decoder step, median / min / max over the repetitions, the same
launches in the same process) and mel frames / s of the whole call, for graph replay and eager launches; the one-launch and the
two-launch form of the frame / prenet tail at batch 1 and 8; and the chunk sizes the default was chosen from.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearningexamples_amd.tacotron2.infer import DEFAULT_CHUNK, Tacotron2Synthesizer    # noqa: E402
from deeplearningexamples_amd.tacotron2.model import DEFAULT_CONFIG, Tacotron2             # noqa: E402


def measure(model, text, lengths, dtype, steps, reps, **kw):
    s = Tacotron2Synthesizer(model, compute_dtype=dtype, max_decoder_steps=steps, early_stopping=False, **kw)
    s.time_decoder = True
    s.infer(text, lengths)                                                # capture + warm-up
    dec, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.infer(text, lengths)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dec.append(s.decoder_ms / steps)
    b = text.shape[0]
    return dict(ms_per_step_median=statistics.median(dec), ms_per_step_min=min(dec), ms_per_step_max=max(dec),
                mel_frames_per_s=b * steps / statistics.median(wall), call_ms_median=1e3 * statistics.median(wall), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron2_infer.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = Tacotron2(device=dev, **DEFAULT_CONFIG)
    g = torch.Generator().manual_seed(1)
    rows = []
    for b in (1, 4, 8):
        text = torch.randint(1, 148, (b, 128), generator=g).to(dev)
        lengths = torch.full((b,), 128, dtype=torch.int64, device=dev)
        for dtype, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            for graph in (True, False):
                rows.append(dict(batch=b, dtype=tag, graph=graph, fused_tail=False, chunk=DEFAULT_CHUNK,
                                 **measure(model, text, lengths, dtype, a.steps, a.reps, graph=graph)))
                print(json.dumps(rows[-1]), flush=True)
            if b in (1, 8):
                for graph in (True, False):
                    rows.append(dict(batch=b, dtype=tag, graph=graph, fused_tail=True, chunk=DEFAULT_CHUNK,
                                     **measure(model, text, lengths, dtype, a.steps, a.reps, graph=graph, fused_tail=True)))
                    print(json.dumps(rows[-1]), flush=True)
        if b in (1, 8):
            for chunk in (2, 8, 32, 64):
                rows.append(dict(batch=b, dtype="fp16", graph=True, fused_tail=False, chunk=chunk,
                                 **measure(model, text, lengths, torch.float16, a.steps, a.reps, chunk=chunk)))
                print(json.dumps(rows[-1]), flush=True)
    out = dict(tool="tools/tacotron2_infer_perf.py", device=torch.cuda.get_device_name(0), steps=a.steps, input_symbols=128,
               widths="default", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
