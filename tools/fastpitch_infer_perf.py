"""FastPitch (default configuration) inference timing on the MI355X: the packed convolution per layer shape against the existing
batched kernel, and the whole synthesizer.

    python tools/fastpitch_infer_perf.py [--reps 30] [--out profiles/fastpitch_infer_perf.json]

Per conv shape of the default configuration -- the FFT block's 384 -> 1536 and 1536 -> 384 (k 3), the predictors' 384 -> 256 and
256 -> 256 (k 3) -- at L in {128, 800} rows (a long text, a long spectrogram): `packed` = F.conv1d_packed_fwd on the rows as ONE
sequence (B = 1, cu = (0, L)), `batched` = F.conv1d_lrelu_fwd on the same rows as a [1, L, C] tensor: the existing kernel is the
yardstick.  The same operands, slope 0 (the ReLU form), no addend; the two outputs are compared bit for bit before anything is
timed.  Two legs in one process, interleaved call by call, every sample one call between two device events after 5 warm-up calls
each; reported: median / average / minimum ms of both legs, packed / batched on the medians, and `spread_pct` of each leg (median of
the even against the odd samples: the run-to-run noise a difference has to beat).  A third leg, `packed_b8`, runs the packed kernel on
8 L rows as 8 sequences of L (what a batch looks like) and is reported per row against the B = 1 figure.

Whole synthesizer: seeded random weights (N(0, 1 / fan_in): finite, nothing trained), seeded random texts of 20 - 160 symbols at
batch 1, 8 and 64, fp16.  The durations are GIVEN (dur_tgt: seeded integers 1 .. 6 per symbol, mean 3.5 frames, at most 960 frames
per utterance): random weights would predict arbitrary lengths, and the 1024-frame envelope must hold.  Reported: latency (one
infer() call between host timestamps around a device synchronisation, as the command line measures it), mel frames / s, and the
share of device time per kernel family from one extra pass under the library's per-launch event timer.

For context only, the reference's README (FastPitch, TorchScript, FP16, DGX A100 1x A100 80GB, 128-character input): batch 1 / 4 / 8:
0.005 / 0.006 / 0.008 s and 120,333 / 424,053 / 669,549 frames/s.  Another GPU, another input, trained weights, padded frames
counted: not a comparison.

The driver touches no GPU.  It starts one child process per measurement group under its own `timeout`, one after the other (never
two GPU processes); a child that fails, faults or runs out of time ends the run (nothing more is started on the GPU).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_SHAPES = [("fft conv 1", 384, 1536, 3), ("fft conv 2", 1536, 384, 3), ("predictor conv 1", 384, 256, 3), ("predictor conv 2", 256, 256, 3)]
ROWS = (128, 800)
BATCHES = (1, 8, 64)
A100_README = dict(source="SpeechSynthesis/FastPitch/README.md, FastPitch (TorchScript, denoising), FP16, 1x A100 80GB, 128 characters",
                   batch=[1, 4, 8], latency_s=[0.005, 0.006, 0.008], frames_per_s=[120333, 424053, 669549])
FAMILIES = (("dle_conv1d_packed_fwd", "packed conv"), ("dle_gemm", "gemm"), ("dle_attention_fwd_varlen", "attention"),
            ("dle_layernorm_fwd", "layernorm"), ("dle_fp_", "fastpitch row kernels"))


def summarise(ms):
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2])
    return dict(avg_ms=sum(ms) / len(ms), median_ms=statistics.median(ms), min_ms=min(ms),
                spread_pct=100.0 * abs(even - odd) / min(even, odd))


def timed(legs, reps):
    import torch
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return ms


def conv_worker(args):
    import torch
    from deeplearningexamples_amd import functional as F
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    rows = []
    for (name, c, ko, ks) in CONV_SHAPES:
        for n in ROWS:
            g = torch.Generator(device=dev).manual_seed(c + ko + n)
            x = torch.randn((8 * n, c), generator=g, device=dev).to(dtype)
            w = (torch.randn((ko, ks, c), generator=g, device=dev) * (ks * c) ** -0.5).to(dtype)
            bias = torch.randn((ko,), generator=g, device=dev) * 0.1
            x1 = x[:n].contiguous()
            cu1 = torch.tensor([0, n], dtype=torch.int32, device=dev)
            cu8 = torch.arange(9, dtype=torch.int32, device=dev) * n
            y1, y2 = torch.empty((n, ko), dtype=dtype, device=dev), torch.empty((1, n, ko), dtype=dtype, device=dev)
            y8 = torch.empty((8 * n, ko), dtype=dtype, device=dev)
            legs = {"packed": lambda: F.conv1d_packed_fwd(x1, w, bias, cu1, n, slope=0.0, out=y1),
                    "batched": lambda: F.conv1d_lrelu_fwd(x1.view(1, n, c), w, bias, slope=0.0, out=y2),
                    "packed_b8": lambda: F.conv1d_packed_fwd(x, w, bias, cu8, n, slope=0.0, out=y8)}
            for fn in legs.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            same = bool(torch.equal(y1.view(torch.int16), y2.view(n, ko).view(torch.int16))) and \
                bool(torch.equal(y8[:n].view(torch.int16), y1.view(torch.int16)))
            ms = timed(legs, args.reps)
            sp, sb, s8 = summarise(ms["packed"]), summarise(ms["batched"]), summarise(ms["packed_b8"])
            rows.append(dict(layer=name, C=c, Ko=ko, ksize=ks, rows=n, dtype=args.amp_dtype, reps=args.reps, bits_equal=same,
                             gflop=2e-9 * n * ko * ks * c, packed=sp, batched=sb, packed_b8=s8,
                             packed_over_batched=sp["median_ms"] / sb["median_ms"],
                             b8_per_row_over_b1=s8["median_ms"] / (8 * sp["median_ms"]),
                             packed_tflops=2e-9 * n * ko * ks * c / sp["median_ms"], b8_tflops=2e-9 * 8 * n * ko * ks * c / s8["median_ms"]))
    print("RESULT " + json.dumps(rows), flush=True)


def random_model(seed=0):
    import numpy as np
    import torch
    from deeplearningexamples_amd.fastpitch.model import DEFAULT_CONFIG, FastPitchModel, state_shapes
    rs = np.random.RandomState(seed)
    state = {}
    for k, shape in state_shapes(DEFAULT_CONFIG).items():
        leaf = k.rsplit(".", 1)[-1]
        if k in ("pitch_mean", "pitch_std"):
            v = np.zeros(shape)
        elif ".layer_norm." in k or ".norm." in k:
            v = np.ones(shape) if leaf == "weight" else np.zeros(shape)
        elif leaf == "bias":
            v = np.zeros(shape)
        elif k.endswith("word_emb.weight"):
            v = rs.standard_normal(shape)
        else:
            v = rs.standard_normal(shape) * int(np.prod(shape[1:])) ** -0.5
        state[k] = torch.from_numpy(np.asarray(v)).float()
    return FastPitchModel(DEFAULT_CONFIG).load_state_dict(state)


def net_worker(args):
    import numpy as np
    import torch
    from deeplearningexamples_amd import _cabi as C
    from deeplearningexamples_amd.fastpitch.infer import FastPitchSynthesizer
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    synth = FastPitchSynthesizer(random_model(), dtype=dtype, device=dev)
    rows = []
    for b in BATCHES:
        rs = np.random.RandomState(100 + b)
        lens = sorted((int(n) for n in rs.randint(20, 161, size=b)), reverse=True)
        texts = [torch.from_numpy(rs.randint(1, 148, size=n)).long().to(dev) for n in lens]
        dur = torch.zeros((b, max(lens)))
        for i, n in enumerate(lens):
            dur[i, :n] = torch.from_numpy(rs.randint(1, 7, size=n)).float()
        dur = dur.to(dev)
        for _ in range(5):
            mel, mel_lens = synth.infer(texts, dur_tgt=dur)[:2]
        torch.cuda.synchronize()
        frames = int(mel_lens.sum())
        finite = bool(torch.isfinite(mel).all())
        lat = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            synth.infer(texts, dur_tgt=dur)
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t0) * 1e3)
        timer = C.KernelTimer()
        C.set_timer(timer)
        synth.infer(texts, dur_tgt=dur)
        C.set_timer(None)
        rep = timer.report()
        total = sum(r["ms"] for r in rep)
        fam = {}
        for r in rep:
            label = next((lab for pre, lab in FAMILIES if r["name"].startswith(pre)), "other")
            fam[label] = fam.get(label, 0.0) + r["ms"]
        s = summarise(lat)
        rows.append(dict(dtype=args.amp_dtype, batch=b, symbols=sum(lens), frames=frames, longest_frames=int(mel_lens.max()), reps=args.reps,
                         finite=finite, latency=s, frames_per_s=frames * 1000.0 / s["median_ms"],
                         padded_frames_per_s=b * int(mel_lens.max()) * 1000.0 / s["median_ms"],
                         launches=sum(r["calls"] for r in rep), device_ms_under_timer=total,
                         share_pct={k: 100.0 * v / total for k, v in sorted(fam.items(), key=lambda kv: -kv[1])}))
    print("RESULT " + json.dumps(rows), flush=True)


def tables(convs, nets):
    lines = ["| layer | C | Ko | rows | packed ms | batched ms | packed / batched | spread % (p, b) | 8 x rows ms | per row vs B = 1 | TFLOP/s (B = 1, 8) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in convs:
        lines.append("| %s | %d | %d | %d | %.4f | %.4f | %.3f | %.1f, %.1f | %.4f | %.2f | %.1f, %.1f |" % (
            r["layer"], r["C"], r["Ko"], r["rows"], r["packed"]["median_ms"], r["batched"]["median_ms"], r["packed_over_batched"],
            r["packed"]["spread_pct"], r["batched"]["spread_pct"], r["packed_b8"]["median_ms"], r["b8_per_row_over_b1"],
            r["packed_tflops"], r["b8_tflops"]))
    lines += ["", "| dtype | batch | symbols | frames | latency ms (median) | spread % | frames/s | launches | share of device time |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in nets:
        lines.append("| %s | %d | %d | %d | %.3f | %.1f | %.3g | %d | %s |" % (
            r["dtype"], r["batch"], r["symbols"], r["frames"], r["latency"]["median_ms"], r["latency"]["spread_pct"], r["frames_per_s"],
            r["launches"], ", ".join("%s %.0f %%" % kv for kv in r["share_pct"].items())))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", default=30, type=int)
    ap.add_argument("--timeout", default=240, type=int, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastpitch_infer_perf.json"))
    ap.add_argument("--worker", default=None, choices=["conv", "net"], help=argparse.SUPPRESS)
    ap.add_argument("--amp-dtype", default="fp16", choices=["bf16", "fp16"])
    args = ap.parse_args()
    if args.worker == "conv":
        return conv_worker(args)
    if args.worker == "net":
        return net_worker(args)
    convs, nets, stopped = [], [], None
    for kind in ("conv", "net"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", kind, "--amp-dtype",
               args.amp_dtype, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            stopped = dict(job=kind, returncode=r.returncode, stderr=r.stderr[-2000:])
            print("%s: child ended with status %d; the run stops here\n%s" % (kind, r.returncode, r.stderr[-2000:]), flush=True)
            break
        (convs if kind == "conv" else nets).extend(json.loads(res[-1][len("RESULT "):]))
        print("%s done" % kind, flush=True)
    print(tables(convs, nets))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(tool="tools/fastpitch_infer_perf.py", conv=convs, network=nets, a100_readme_for_context=A100_README, stopped=stopped),
              open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
