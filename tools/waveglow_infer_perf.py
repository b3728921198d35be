"""The `-m WaveGlow --synth-data` leg of the reference's inference_perf.py for the HIP vocoder: one normal(-5.62, 1.98)
spectrogram [1, 80, 895], 6 warm-up calls, then device-event timing of --calls (>= 20) calls of WaveGlowVocoder.infer; and, in
the same run, WaveGlowTrainer.forward on the same spectrogram and number of samples (same M rows) for comparison.

    python tools/waveglow_infer_perf.py [--amp-dtype fp16|bf16] [--calls 20] [--out FILE.json]

Prints one JSON line: infer_latency (s, mean), infer_items_per_sec (audio samples / s), the spread, train_forward_latency.
Freshly initialised weights (end = 0 does not change the work done).  Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sorted(s.elapsed_time(e) * 1e-3 for s, e in ev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=895)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--sigma-infer", type=float, default=0.9)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.calls < 20:
        raise SystemExit("--calls: at least 20")
    from deeplearningexamples_amd.waveglow.engine import WaveGlowTrainer
    from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
    from deeplearningexamples_amd.waveglow.inference import synth_mel
    from deeplearningexamples_amd.waveglow.model import DEFAULT_CONFIG, WaveGlow
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    torch.manual_seed(0)
    model = WaveGlow(**DEFAULT_CONFIG, device=dev)
    mel = synth_mel(1, 80, args.frames, 0).to(dev)
    samples = args.frames * 256
    voc = WaveGlowVocoder(model, compute_dtype=dt)
    for _ in range(args.warmup):
        voc.infer(mel, sigma=args.sigma_infer)
    t = timed(lambda: voc.infer(mel, sigma=args.sigma_infer), args.calls)
    res = {"model": "WaveGlow", "dtype": args.amp_dtype, "mel": [1, 80, args.frames], "samples": samples, "calls": args.calls,
           "warmup": args.warmup, "infer_latency": sum(t) / len(t), "infer_latency_min": t[0], "infer_latency_median": t[len(t) // 2],
           "infer_latency_max": t[-1], "infer_items_per_sec": samples * len(t) / sum(t)}
    peak0 = torch.cuda.max_memory_allocated()
    del voc
    torch.cuda.empty_cache()
    # the train step's forward at the same M: same GEMMs + the loss, and it keeps what a backward pass needs
    tr = WaveGlowTrainer(model, compute_dtype=dt)
    audio = (torch.randn(1, samples, device=dev) * 0.2).clamp_(-1, 1)
    for _ in range(2):
        tr.forward(mel, audio)
    tf = timed(lambda: tr.forward(mel, audio), 5)
    res.update({"train_forward_latency": sum(tf) / len(tf), "train_forward_latency_min": tf[0], "train_forward_calls": len(tf),
                "infer_peak_bytes": peak0})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
