"""EfficientNet inference timing on the MI355X: the depthwise kernel per layer shape against its byte bound, and whole networks.

    python tools/efficientnet_infer_perf.py [--reps 30] [--out profiles/efficientnet_infer_perf.json]

Per layer: every distinct depthwise shape (H, W, C, k, stride) of efficientnet-b0 at 224 x 224 and efficientnet-b4 at 380 x 380,
each at batch 1, 32 and 256.  Two legs in one process, interleaved call by call, every sample one call between two device events,
three warm-up calls per leg first: `kernel` = F.dwconv2d_act_fwd with both SiLUs and the pool partials (what the classifier
launches), `torch` = the torch composition of the same math on the same tensors (silu, F.conv2d(groups=C) on a channels_last view,
batch_norm, silu, mean).  The two outputs are compared before anything is timed.  Reported: median / average ms of both legs, the
kernel's byte bound = (input + output + pool bytes) / 6.29 TB/s (the measured copy rate of the device) and the kernel's time over
it, and `spread_pct` (medians of the even against the odd samples of the same leg: the noise a difference has to beat).  No ratio
is asserted anywhere.

Whole network: latency and images / s at batch 1, 2, ..., 256, b0 and b4 at their own image sizes, both 16-bit types, eager and
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

LAYER_BATCHES = (1, 32, 256)
NET_BATCHES = (1, 2, 4, 8, 16, 32, 64, 128, 256)
ARCHS = ("efficientnet-b0", "efficientnet-b4")
COPY_RATE = 6.29e12          # bytes / s, measured copy


def depthwise_shapes(arch_name):
    """The distinct (H, W, C, k, stride) of the architecture's depthwise units at its own image size, in network order."""
    from deeplearningexamples_amd.convnets import efficientnet as E
    arch = E.ARCHS[arch_name]
    h = (arch.default_image_size - 1) // 2 + 1
    out = []
    for (_, _, k, s, cin, _, e) in arch.blocks():
        shape = (h, h, cin * e, k, s)
        if shape not in out:
            out.append(shape)
        h = (h - 1) // s + 1
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
    from deeplearningexamples_amd.utils.state import fold_bn
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    tf = torch.nn.functional
    rows = []
    for (h, w, c, k, stride) in depthwise_shapes(args.arch):
        for n in LAYER_BATCHES:
            g = torch.Generator(device=dev).manual_seed(h * 1000 + c + n)
            x = torch.randn((n, h, w, c), generator=g, device=dev).to(dtype)
            wt = (torch.randn((c, 1, k, k), generator=g, device=dev) / k).to(dtype)
            wp = F.pack_depthwise_weight(wt, dtype)
            gamma, beta = torch.rand((c,), generator=g, device=dev) + 0.5, torch.randn((c,), generator=g, device=dev) * 0.1
            mean, var = torch.randn((c,), generator=g, device=dev) * 0.1, torch.rand((c,), generator=g, device=dev) + 0.5
            scale, shift = fold_bn(gamma, beta, mean, var, 1e-3)
            y = torch.empty((n, (h - 1) // stride + 1, (w - 1) // stride + 1, c), dtype=dtype, device=dev)
            pool = torch.empty((n, F.dwconv2d_pool_bands(h, w, c, k, stride), c), dtype=torch.float32, device=dev)
            xv = x.permute(0, 3, 1, 2)                  # the same memory as an NCHW tensor in channels_last
            keep = {}

            def composed():
                t = tf.silu(tf.batch_norm(tf.conv2d(tf.silu(xv), wt, None, stride, k // 2, 1, c), mean, var, gamma, beta, False, 0.0, 1e-3))
                keep["y"], keep["mean"] = t, t.float().mean((2, 3))
            legs = {"kernel": lambda: F.dwconv2d_act_fwd(x, wp, scale, shift, stride, in_act=True, out_act=True, pool=pool, out=y),
                    "torch": composed}
            for fn in legs.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            diff = float((y.float() - keep["y"].permute(0, 2, 3, 1).float()).abs().max())
            mean_diff = float((pool.sum(1) / (y.shape[1] * y.shape[2]) - keep["mean"]).abs().max())
            ms = timed(legs, args.reps)
            sk, st = summarise(ms["kernel"]), summarise(ms["torch"])
            nbytes = 2.0 * (x.numel() + y.numel()) + 4.0 * pool.numel()
            bound_ms = nbytes / COPY_RATE * 1e3
            rows.append(dict(arch=args.arch, shape="%dx%dx%d k%d s%d" % (h, w, c, k, stride), batch=n, dtype=args.amp_dtype, reps=args.reps,
                             max_abs_diff=diff, max_abs_mean_diff=mean_diff, max_abs_out=float(y.float().abs().max()),
                             algorithmic_bytes=nbytes, byte_bound_ms=bound_ms, kernel=sk, torch=st,
                             kernel_over_bound=sk["median_ms"] / bound_ms, torch_over_kernel=st["median_ms"] / sk["median_ms"]))
            del x, y, pool, xv, keep
    print("RESULT " + json.dumps(rows), flush=True)


def net_worker(args):
    import torch
    from deeplearningexamples_amd.convnets import efficientnet as E
    from deeplearningexamples_amd.convnets.infer import EfficientNetClassifier
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    torch.manual_seed(0)
    model = E.build(args.arch, device=dev)
    size = args.image_size or E.ARCHS[args.arch].default_image_size
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for blk in model.mbconv_blocks():         # a small projection gamma keeps the residual chains inside fp16
            blk.proj.bn.weight.data.copy_(torch.rand(blk.proj.bn.num_features, generator=g) * 0.25 + 0.125)
    eager = EfficientNetClassifier(model, dtype=dtype)
    graphed = EfficientNetClassifier(model, dtype=dtype, graphs=True)
    rows = []
    for b in [int(v) for v in args.batches.split(",")]:
        images = torch.randn((b, 3, size, size), generator=torch.Generator().manual_seed(2)).to(dev)
        legs = {"eager": lambda: eager.logits(images), "graph": lambda: graphed.logits(images)}
        for fn in legs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(legs["eager"]()).all())
        same = bool(torch.equal(legs["eager"](), legs["graph"]()))
        ms = timed(legs, args.reps)
        row = dict(arch=args.arch, dtype=args.amp_dtype, batch=b, image_size=size, reps=args.reps, finite=finite, graph_equals_eager=same)
        for k, v in ms.items():
            row[k] = summarise(v)
            row[k]["img_per_s"] = b * 1000.0 / row[k]["avg_ms"]
        rows.append(row)
        del images
    print("RESULT " + json.dumps(rows), flush=True)


def tables(layers, nets):
    lines = ["| arch | shape | batch | dtype | kernel ms | byte bound ms | kernel / bound | torch ms | torch / kernel | spread % (k, t) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in layers:
        lines.append("| %s | %s | %d | %s | %.4f | %.4f | %.2f | %.4f | %.2f | %.1f, %.1f |" % (
            r["arch"], r["shape"], r["batch"], r["dtype"], r["kernel"]["median_ms"], r["byte_bound_ms"], r["kernel_over_bound"],
            r["torch"]["median_ms"], r["torch_over_kernel"], r["kernel"]["spread_pct"], r["torch"]["spread_pct"]))
    lines += ["", "| arch | dtype | image | batch | eager ms | eager img/s | graph ms | graph img/s |", "|---|---|---|---|---|---|---|---|"]
    for r in nets:
        lines.append("| %s | %s | %d | %d | %.3f | %.0f | %.3f | %.0f |" % (r["arch"], r["dtype"], r["image_size"], r["batch"], r["eager"]["avg_ms"],
                                                                            r["eager"]["img_per_s"], r["graph"]["avg_ms"], r["graph"]["img_per_s"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", default=30, type=int)
    ap.add_argument("--image-size", default=0, type=int, help="whole networks: 0 = the architecture's own size")
    ap.add_argument("--batches", default=",".join(map(str, NET_BATCHES)))
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--skip-networks", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--timeout", default=240, type=int, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efficientnet_infer_perf.json"))
    ap.add_argument("--worker", default=None, choices=["layers", "net"], help=argparse.SUPPRESS)
    ap.add_argument("--arch", default=ARCHS[0], help=argparse.SUPPRESS)
    ap.add_argument("--amp-dtype", default="bf16", choices=["bf16", "fp16"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "layers":
        return layer_worker(args)
    if args.worker == "net":
        return net_worker(args)
    dts = args.dtypes.split(",")
    jobs = [] if args.skip_layers else [("layers", arch, dt) for arch in ARCHS for dt in dts]
    if not args.skip_networks:
        jobs += [("net", arch, dt) for arch in ARCHS for dt in dts]
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
        print("%s %s %s done" % (kind, arch, dt), flush=True)
    print(tables(layers, nets))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(tool="tools/efficientnet_infer_perf.py", copy_rate_bytes_per_s=COPY_RATE, layers=layers, networks=nets, stopped=stopped),
              open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
