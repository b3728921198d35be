"""ResNet-50 inference timing: ResNet50Classifier (BatchNorm in the convolution epilogues) against ResNetTrainer.infer (the parent
path: convolution + BatchNorm-apply, two launches per unit) on the same weights, batch 1, 2, 4, ..., 256 at 224 x 224, synthetic
images -- the reference's benchmark_inference table (Classification/ConvNets/resnet50v1.5/README.md, "Inference performance").

    python tools/rn50_infer_perf.py [--amp-dtype fp16] [--reps 60] [--graphs] [--out profiles/rn50_infer_perf.json]

The driver touches no GPU.  Per batch size it starts ONE child process under its own `timeout`, one after the other (never two GPU
processes); a child that fails, faults or runs out of time ends the sweep (nothing more is started on the GPU).  Inside a child the
legs -- fused, parent (and fused + graph replay with --graphs) -- are timed in one process, interleaved call by call: every sample is
one call between two device events, so both legs see the same clocks and the same neighbours.  Reported per leg: average, p90, p95,
p99 latency (ms) and images / s (batch / average latency), the reference table's columns; and `spread_pct`, the run-to-run spread
the comparison has to beat: the relative difference between the medians of the even and the odd samples of the same leg.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def percentile(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(q / 100.0 * (len(s) - 1))))]


def summarise(ms, batch):
    avg = sum(ms) / len(ms)
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2])
    return dict(avg_ms=avg, median_ms=statistics.median(ms), p90_ms=percentile(ms, 90), p95_ms=percentile(ms, 95),
                p99_ms=percentile(ms, 99), img_per_s=batch * 1000.0 / avg, spread_pct=100.0 * abs(even - odd) / min(even, odd))


def worker(args):
    import torch
    from deeplearningexamples_amd.convnets.engine import ResNetTrainer
    from deeplearningexamples_amd.convnets.infer import ResNet50Classifier
    from deeplearningexamples_amd.convnets.resnet import ResNet50
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    torch.manual_seed(0)
    model = ResNet50(device=dev)
    g = torch.Generator().manual_seed(1)
    for m in model.modules():                     # a non-trivial affine map (the default initialisation zeroes nothing, but is 1 / 0)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.25)
    b = args.batch
    images = torch.randn((b, 3, args.image_size, args.image_size), generator=torch.Generator().manual_seed(2)).to(dev)
    fused = ResNet50Classifier(model, dtype=dtype)
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=dtype)
    legs = {"fused": lambda: fused.logits(images), "parent": lambda: trainer.infer(images)}
    if args.graphs:
        graphed = ResNet50Classifier(model, dtype=dtype, graphs=True)
        legs["fused_graph"] = lambda: graphed.logits(images)
    for fn in legs.values():                      # warm every leg: code objects, allocator, graph capture
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # same weights, same images: the two paths must agree to the 16-bit noise of the network before their times are compared
    diff = float((legs["fused"]() - legs["parent"]()).abs().max())
    scale = float(legs["parent"]().abs().max())
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    out = dict(batch=b, image_size=args.image_size, dtype=args.amp_dtype, reps=args.reps, max_logit_diff=diff, max_logit=scale,
               legs={k: summarise(v, b) for k, v in ms.items()})
    print("RESULT " + json.dumps(out), flush=True)


def table(rows):
    lines = ["| batch | leg | avg ms | p90 ms | p95 ms | p99 ms | img/s | spread % | fused / parent |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for k, v in r["legs"].items():
            ratio = "%.3f" % (v["avg_ms"] / r["legs"]["parent"]["avg_ms"]) if k != "parent" else ""
            lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.0f | %.1f | %s |" % (
                r["batch"], k, v["avg_ms"], v["p90_ms"], v["p95_ms"], v["p99_ms"], v["img_per_s"], v["spread_pct"], ratio))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--image-size", default=224, type=int)
    ap.add_argument("--amp-dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--reps", default=60, type=int)
    ap.add_argument("--graphs", action="store_true")
    ap.add_argument("--timeout", default=150, type=int, help="seconds per batch size (its own child process)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", default=1, type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    rows, stopped = [], None
    for b in [int(x) for x in args.batches.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--batch", str(b),
               "--image-size", str(args.image_size), "--amp-dtype", args.amp_dtype, "--reps", str(args.reps)] + (["--graphs"] if args.graphs else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            stopped = dict(batch=b, returncode=r.returncode, stderr=r.stderr[-2000:])
            print("batch %d: child ended with status %d; the sweep stops here\n%s" % (b, r.returncode, r.stderr[-2000:]), flush=True)
            break
        rows.append(json.loads(res[-1][len("RESULT "):]))
        print("batch %d done" % b, flush=True)
    print(table(rows))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(dict(tool="tools/rn50_infer_perf.py", rows=rows, stopped=stopped), open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
