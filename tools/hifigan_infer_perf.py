"""HiFi-GAN (V1) inference timing on the MI355X: the fused dilated conv1d kernel per layer shape, and the whole network.

    python tools/hifigan_infer_perf.py [--reps 20] [--out profiles/hifigan_infer_perf.json]

Per layer: every (C, Ko, ksize, dilation) the V1 generator runs -- conv_pre (80 -> 512, k 7) at L = T, the four packed upsample
convolutions (k 3) at L = T, 8T, 64T, 128T, and per stage (ch, L) = (256, 8T), (128, 64T), (64, 128T), (32, 256T) the resblock
convolutions k in {3, 7, 11} x dilation in {1, 3, 5} -- for T in {100, 800} mel frames and B in {1, 16}.  Two legs in one process,
interleaved call by call, every sample one call between two device events: `fused` = F.conv1d_lrelu_fwd (slope 0.1, one addend:
the form most launches of the network take), `taps_gemm` = the composition the project could already run, dle_wg_taps into a
[B L, ksize C] column matrix + F.gemm with bias, on PRE-ACTIVATED input and without the addend (so it does less).  The two outputs
are compared (on pre-activated input, no addend) before anything is timed.  Reported: median / average ms of both legs, `floor_ms`
= the bytes the fused launch must move (x, w, the addend and y, 16-bit, each once) / 6.3 TB/s (the rate a streaming kernel
reaches here), fused / floor, taps_gemm / fused, and `spread_pct` (medians of the even against the odd
samples of the same leg: the noise a difference has to beat).  Operands of the small shapes fit in the caches: their floor is not an HBM floor, and is marked
`in_cache` when x + y + addend stay below 64 MB.

Whole network: audio samples / s and the multiple of real time (22,050 Hz) at T in {100, 800} and B in {1, 16}, fp16, eager and
graph replay.

The driver touches no GPU.  It starts one child process per measurement group under its own `timeout`, one after the other (never
two GPU processes); a child that fails, faults or runs out of time ends the run (nothing more is started on the GPU).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
FRAMES = (100, 800)
BATCHES = (1, 16)
SAMPLING_RATE = 22050


def layer_shapes():
    """[(name, C, Ko, ksize, dilation, L / T)] of the V1 generator."""
    out = [("conv_pre", 80, 512, 7, 1, 1), ("ups.0 (packed)", 512, 8 * 256, 3, 1, 1), ("ups.1 (packed)", 256, 8 * 128, 3, 1, 8),
           ("ups.2 (packed)", 128, 2 * 64, 3, 1, 64), ("ups.3 (packed)", 64, 2 * 32, 3, 1, 128)]
    for ch, mult in ((256, 8), (128, 64), (64, 128), (32, 256)):
        for k in (3, 7, 11):
            for d in (1, 3, 5):
                out.append(("resblock", ch, ch, k, d, mult))
    return out


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


def layer_worker(args):
    import torch
    from deeplearningexamples_amd import functional as F
    from deeplearningexamples_amd.waveglow import ops
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    t, b = args.frames, args.batch
    rows = []
    for (name, c, ko, ks, dil, mult) in layer_shapes():
        steps = t * mult
        g = torch.Generator(device=dev).manual_seed(c * 100 + ks * 10 + dil)
        x = torch.randn((b, steps, c), generator=g, device=dev).to(dtype)
        w = (torch.randn((ko, ks, c), generator=g, device=dev) * (ks * c) ** -0.5).to(dtype)
        bias = torch.randn((ko,), generator=g, device=dev) * 0.1
        add = torch.randn((b, steps, ko), generator=g, device=dev).to(dtype)
        a = torch.where(x < 0, (x.float() * 0.1).to(dtype), x)            # the pre-activated input of the composition
        y, y2 = torch.empty((b, steps, ko), dtype=dtype, device=dev), torch.empty((b * steps, ko), dtype=dtype, device=dev)
        col = torch.empty((b * steps, ks * c), dtype=dtype, device=dev)
        w2 = w.view(ko, ks * c)

        def taps_gemm():
            ops.taps(a.view(b * steps, c), b, steps, ks, dil, ks // 2, out=col)
            F.gemm(col, w2, b * steps, ko, ks * c, True, True, bias=bias, out=y2)
        legs = {"fused": lambda: F.conv1d_lrelu_fwd(x, w, bias, dilation=dil, slope=0.1, add1=add, out=y), "taps_gemm": taps_gemm}
        F.conv1d_lrelu_fwd(a, w, bias, dilation=dil, out=y)               # same math as the composition: compare first
        taps_gemm()
        torch.cuda.synchronize()
        diff = float((y.view(b * steps, ko).float() - y2.float()).abs().max())
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = timed(legs, args.reps)
        sf, sg = summarise(ms["fused"]), summarise(ms["taps_gemm"])
        nbytes = 2.0 * (x.numel() + w.numel() + 2 * y.numel())
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        rows.append(dict(layer=name, C=c, Ko=ko, ksize=ks, dilation=dil, L=steps, frames=t, batch=b, dtype=args.amp_dtype, reps=args.reps,
                         max_abs_diff=diff, max_abs_out=float(y2.float().abs().max()), gflop=2e-9 * b * steps * ko * ks * c,
                         algorithmic_bytes=nbytes, in_cache=bool(2.0 * (x.numel() + 2 * y.numel()) < 64e6), floor_ms=floor_ms,
                         fused=sf, taps_gemm=sg, fused_over_floor=sf["median_ms"] / floor_ms,
                         taps_gemm_over_fused=sg["median_ms"] / sf["median_ms"]))
        del x, w, add, a, y, y2, col
    print("RESULT " + json.dumps(rows), flush=True)


def net_worker(args):
    import torch
    from deeplearningexamples_amd.hifigan.infer import HifiGanVocoder
    from deeplearningexamples_amd.hifigan.model import V1_CONFIG, HifiGanGenerator, layers
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(0)
    state = {}
    for l in layers(V1_CONFIG):                                            # N(0, 1 / fan_in) weights: finite audio, nothing trained
        shape, fan = ((l.cout, l.cin, l.ksize), l.ksize * l.cin) if l.kind == "conv" else ((l.cin, l.cout, l.ksize), l.ksize * l.cin / l.stride)
        v = torch.randn(shape, generator=g) * fan ** -0.5
        state[l.name + ".weight_v"], state[l.name + ".bias"] = v, torch.zeros(l.cout)
        state[l.name + ".weight_g"] = torch.linalg.vector_norm(v, 2, dim=(1, 2), keepdim=True)
    model = HifiGanGenerator(V1_CONFIG).load_state_dict(state)
    eager, graphed = HifiGanVocoder(model, dtype=dtype, device=dev), HifiGanVocoder(model, dtype=dtype, device=dev, graphs=True)
    rows = []
    for t in FRAMES:
        for b in BATCHES:
            mel = torch.randn((b, 80, t), generator=torch.Generator().manual_seed(1)).to(dev)
            legs = {"eager": lambda: eager.infer(mel), "graph": lambda: graphed.infer(mel)}
            for fn in legs.values():
                for _ in range(4):
                    fn()
            torch.cuda.synchronize()
            finite = bool(torch.isfinite(legs["eager"]()).all())
            same = bool(torch.equal(legs["eager"](), legs["graph"]()))
            ms = timed(legs, args.reps)
            row = dict(dtype=args.amp_dtype, batch=b, frames=t, samples=b * t * 256, reps=args.reps, finite=finite, graph_equals_eager=same)
            for k, v in ms.items():
                row[k] = summarise(v)
                row[k]["samples_per_s"] = b * t * 256 * 1000.0 / row[k]["avg_ms"]
                row[k]["x_real_time"] = row[k]["samples_per_s"] / SAMPLING_RATE
            rows.append(row)
            del mel
    print("RESULT " + json.dumps(rows), flush=True)


def tables(layers, nets):
    lines = ["| layer | C | Ko | k | d | B | L | fused ms | floor ms | fused / floor | taps+gemm ms | taps+gemm / fused | spread % (f, t) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in layers:
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %.4f | %.4f%s | %.1f | %.4f | %.2f | %.1f, %.1f |" % (
            r["layer"], r["C"], r["Ko"], r["ksize"], r["dilation"], r["batch"], r["L"], r["fused"]["median_ms"], r["floor_ms"],
            " (cache)" if r["in_cache"] else "", r["fused_over_floor"], r["taps_gemm"]["median_ms"], r["taps_gemm_over_fused"],
            r["fused"]["spread_pct"], r["taps_gemm"]["spread_pct"]))
    lines += ["", "| dtype | batch | frames | eager ms | eager samples/s | x real time | graph ms | graph samples/s | x real time |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in nets:
        lines.append("| %s | %d | %d | %.3f | %.3g | %.0f | %.3f | %.3g | %.0f |" % (
            r["dtype"], r["batch"], r["frames"], r["eager"]["avg_ms"], r["eager"]["samples_per_s"], r["eager"]["x_real_time"],
            r["graph"]["avg_ms"], r["graph"]["samples_per_s"], r["graph"]["x_real_time"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", default=20, type=int)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--timeout", default=240, type=int, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hifigan_infer_perf.json"))
    ap.add_argument("--worker", default=None, choices=["layers", "net"], help=argparse.SUPPRESS)
    ap.add_argument("--frames", default=100, type=int, help=argparse.SUPPRESS)
    ap.add_argument("--batch", default=1, type=int, help=argparse.SUPPRESS)
    ap.add_argument("--amp-dtype", default="fp16", choices=["bf16", "fp16"])
    args = ap.parse_args()
    if args.worker == "layers":
        return layer_worker(args)
    if args.worker == "net":
        return net_worker(args)
    jobs = [] if args.skip_layers else [("layers", t, b) for t in FRAMES for b in BATCHES]
    if not args.skip_network:
        jobs.append(("net", 0, 0))
    layers, nets, stopped = [], [], None
    for kind, t, b in jobs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", kind, "--frames", str(t),
               "--batch", str(b), "--amp-dtype", args.amp_dtype, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            stopped = dict(job=[kind, t, b], returncode=r.returncode, stderr=r.stderr[-2000:])
            print("%s T=%d B=%d: child ended with status %d; the run stops here\n%s" % (kind, t, b, r.returncode, r.stderr[-2000:]), flush=True)
            break
        (layers if kind == "layers" else nets).extend(json.loads(res[-1][len("RESULT "):]))
        print("%s T=%d B=%d done" % (kind, t, b), flush=True)
    print(tables(layers, nets))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(tool="tools/hifigan_infer_perf.py", hbm_bytes_per_s=HBM_BYTES_PER_S, layers=layers, network=nets, stopped=stopped),
              open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
