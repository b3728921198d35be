"""(SE-)ResNeXt101-32x4d inference timing on the MI355X: the grouped 3x3 kernel per layer shape, and whole networks.

    python tools/resnext_infer_perf.py [--reps 30] [--out profiles/resnext_infer_perf.json]

Per layer: the seven grouped shapes of the network at 224 x 224 (stride 1: 56x56x128, 28x28x256, 14x14x512, 7x7x1024; stride 2:
56->28 x256, 28->14 x512, 14->7 x1024), each at batch 32 and 256.  Two legs in one process, interleaved call by call, every sample
one call between two device events: `grouped` = F.conv2d_grouped_fwd_affine, `dense` = the parent's path for the same math,
F.conv2d_fwd_affine on block-diagonal zero-expanded dense weights [Ko,3,3,C].  The two outputs are compared before anything is
timed.  Reported: median / average ms of both legs, the grouped kernel's GB/s over ALGORITHMIC bytes (x + grouped w + y, 16-bit,
each once), dense / grouped, and `spread_pct` (medians of the even against the odd samples of the same leg: the noise a difference
has to beat).

Whole network: latency and images / s at batch 1, 2, ..., 256, both architectures and both 16-bit types, eager and graph replay.

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

# (H, W, C, stride): conv2 of the four stages, and of the first block of stages 2-4
LAYERS = ((56, 56, 128, 1), (28, 28, 256, 1), (14, 14, 512, 1), (7, 7, 1024, 1), (56, 56, 256, 2), (28, 28, 512, 2), (14, 14, 1024, 2))
LAYER_BATCHES = (32, 256)
NET_BATCHES = (1, 2, 4, 8, 16, 32, 64, 128, 256)
ARCHS = ("resnext101-32x4d", "se-resnext101-32x4d")
GROUPS = 32


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


def expand_dense(w, groups):
    """[Ko,3,3,Cg] grouped -> [Ko,3,3,C] block-diagonal dense (zeros outside ko's group)."""
    import torch
    ko, _, _, cg = w.shape
    kg = ko // groups
    d = torch.zeros((ko, 3, 3, cg * groups), dtype=w.dtype, device=w.device)
    for g in range(groups):
        d[g * kg:(g + 1) * kg, :, :, g * cg:(g + 1) * cg] = w[g * kg:(g + 1) * kg]
    return d


def layer_worker(args):
    import torch
    from deeplearningexamples_amd import functional as F
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    rows = []
    for (h, w, c, stride) in LAYERS:
        for n in LAYER_BATCHES:
            g = torch.Generator(device=dev).manual_seed(h * 1000 + c + n)
            cg = c // GROUPS
            x = torch.randn((n, h, w, c), generator=g, device=dev).to(dtype)
            wg = (torch.randn((c, 3, 3, cg), generator=g, device=dev) * (9 * cg) ** -0.5).to(dtype)
            wd = expand_dense(wg, GROUPS)
            scale = torch.rand((c,), generator=g, device=dev) + 0.5
            shift = torch.randn((c,), generator=g, device=dev) * 0.1
            p, q = (h - 1) // stride + 1, (w - 1) // stride + 1
            yg = torch.empty((n, p, q, c), dtype=dtype, device=dev)
            yd = torch.empty_like(yg)
            legs = {"grouped": lambda: F.conv2d_grouped_fwd_affine(x, wg, scale, shift, GROUPS, stride, relu=True, out=yg),
                    "dense": lambda: F.conv2d_fwd_affine(x, wd, scale, shift, stride, 1, relu=True, out=yd)}
            for fn in legs.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            diff = float((yg.float() - yd.float()).abs().max())
            ms = timed(legs, args.reps)
            sg, sd = summarise(ms["grouped"]), summarise(ms["dense"])
            nbytes = 2.0 * (x.numel() + wg.numel() + yg.numel())
            rows.append(dict(shape="%dx%dx%d s%d" % (h, w, c, stride), batch=n, cg=cg, dtype=args.amp_dtype, reps=args.reps,
                             max_abs_diff=diff, max_abs_out=float(yd.float().abs().max()), algorithmic_bytes=nbytes,
                             grouped=sg, dense=sd, grouped_gbps=nbytes / (sg["median_ms"] * 1e-3) / 1e9,
                             dense_over_grouped=sd["median_ms"] / sg["median_ms"]))
            del x, wg, wd, yg, yd
    print("RESULT " + json.dumps(rows), flush=True)


def net_worker(args):
    import torch
    from deeplearningexamples_amd.convnets import resnext
    from deeplearningexamples_amd.convnets.infer import ResNeXtClassifier
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    torch.manual_seed(0)
    model = resnext.build(args.arch, device=dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for blk in model.bottlenecks():           # a small bn3 gamma keeps 33 residual blocks inside fp16
            blk.bn3.weight.data.copy_(torch.rand(blk.bn3.num_features, generator=g) * 0.25 + 0.125)
    eager = ResNeXtClassifier(model, dtype=dtype)
    graphed = ResNeXtClassifier(model, dtype=dtype, graphs=True)
    rows = []
    for b in [int(v) for v in args.batches.split(",")]:
        images = torch.randn((b, 3, args.image_size, args.image_size), generator=torch.Generator().manual_seed(2)).to(dev)
        legs = {"eager": lambda: eager.logits(images), "graph": lambda: graphed.logits(images)}
        for fn in legs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(legs["eager"]()).all())
        same = bool(torch.equal(legs["eager"](), legs["graph"]()))
        ms = timed(legs, args.reps)
        row = dict(arch=args.arch, dtype=args.amp_dtype, batch=b, image_size=args.image_size, reps=args.reps, finite=finite,
                   graph_equals_eager=same)
        for k, v in ms.items():
            row[k] = summarise(v)
            row[k]["img_per_s"] = b * 1000.0 / row[k]["avg_ms"]
        rows.append(row)
        del images
    print("RESULT " + json.dumps(rows), flush=True)


def tables(layers, nets):
    lines = ["| shape | batch | Cg | grouped ms | GB/s | dense-expanded ms | dense / grouped | spread % (g, d) |", "|---|---|---|---|---|---|---|---|"]
    for r in layers:
        lines.append("| %s | %d | %d | %.4f | %.0f | %.4f | %.2f | %.1f, %.1f |" % (
            r["shape"], r["batch"], r["cg"], r["grouped"]["median_ms"], r["grouped_gbps"], r["dense"]["median_ms"], r["dense_over_grouped"],
            r["grouped"]["spread_pct"], r["dense"]["spread_pct"]))
    lines += ["", "| arch | dtype | batch | eager ms | eager img/s | graph ms | graph img/s |", "|---|---|---|---|---|---|---|"]
    for r in nets:
        lines.append("| %s | %s | %d | %.3f | %.0f | %.3f | %.0f |" % (r["arch"], r["dtype"], r["batch"], r["eager"]["avg_ms"],
                                                                       r["eager"]["img_per_s"], r["graph"]["avg_ms"], r["graph"]["img_per_s"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", default=30, type=int)
    ap.add_argument("--image-size", default=224, type=int)
    ap.add_argument("--batches", default=",".join(map(str, NET_BATCHES)))
    ap.add_argument("--skip-networks", action="store_true")
    ap.add_argument("--timeout", default=240, type=int, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnext_infer_perf.json"))
    ap.add_argument("--worker", default=None, choices=["layers", "net"], help=argparse.SUPPRESS)
    ap.add_argument("--arch", default=ARCHS[0], help=argparse.SUPPRESS)
    ap.add_argument("--amp-dtype", default="bf16", choices=["bf16", "fp16"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "layers":
        return layer_worker(args)
    if args.worker == "net":
        return net_worker(args)
    jobs = [("layers", ARCHS[0], dt) for dt in ("bf16", "fp16")]
    if not args.skip_networks:
        jobs += [("net", arch, dt) for arch in ARCHS for dt in ("bf16", "fp16")]
    layers, nets, stopped = [], [], None
    for kind, arch, dt in jobs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", kind, "--arch", arch,
               "--amp-dtype", dt, "--reps", str(args.reps), "--image-size", str(args.image_size), "--batches", args.batches]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            stopped = dict(job=[kind, arch, dt], returncode=r.returncode, stderr=r.stderr[-2000:])
            print("%s %s %s: child ended with status %d; the run stops here\n%s" % (kind, arch, dt, r.returncode, r.stderr[-2000:]), flush=True)
            break
        (layers if kind == "layers" else nets).extend(json.loads(res[-1][len("RESULT "):]))
        print("%s %s %s done" % (kind, arch if kind == "net" else "", dt), flush=True)
    print(tables(layers, nets))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(tool="tools/resnext_infer_perf.py", layers=layers, networks=nets, stopped=stopped), open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
