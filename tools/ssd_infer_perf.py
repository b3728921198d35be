"""SSD300 inference timing on the MI355X: the network, the network with the detection, the post-processing against the reference
algorithm's Python loop, and the head convolutions at two output paddings.

    python tools/ssd_infer_perf.py [--reps 20] [--out profiles/ssd_infer_perf.json]

net    the published-size network (width 1, random weights, BatchNorm randomised as the tests do) at 300 x 300, batch 1, 8 and 32,
       fp16 and bf16: `network` = SSDDetector.head_outputs (what the reference's benchmark-inference times: the forward alone),
       `detect` = SSDDetector.detect (the forward, decode, NMS and selection), each eager and as a graph replay.  Four legs
       interleaved call by call in one process, every sample one call between two device events, four warm-up calls per leg.
post   the post-processing alone at batch 32 on detector-like outputs (tests/_ssd_ref.case_inputs: background-dominated logits,
       clusters of overlapping boxes, one class with 260 candidates): `kernels` = dle_ssd_decode_fwd + dle_ssd_nms_fwd +
       dle_ssd_select_fwd, `nms_select` = the last two, `loop` = the reference algorithm's Python loop (tests/_ssd_ref.decode_ref +
       detect_ref, the torch form of Encoder.decode_batch) on the SAME device tensors.  The loop stands in for the reference,
       which is not part of this repository.  The kernels' detections are compared with the loop's before anything is timed.
heads  the six head launches (3x3 / pad 1, [loc; conf] weights, Ko = nd * 85) with the output channels padded to a multiple of 8
       (344 / 512) against a multiple of 64 (384 / 512), batch 1, 8, 32, interleaved.

`spread_pct` (medians of the even against the odd samples of one leg) is the noise a difference has to beat.  Nothing is asserted.
The driver touches no GPU: one child process per group under its own `timeout`, one after the other; a child that fails, faults
or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 8, 32)


def summarise(ms):
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2]) if len(ms) > 1 else statistics.median(ms)
    return dict(avg_ms=sum(ms) / len(ms), median_ms=statistics.median(ms), min_ms=min(ms), samples=len(ms),
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


def _dtype(args):
    import torch
    return torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16


def _model(width=1):
    import torch
    from deeplearningexamples_amd.ssd import model as M
    from tests import _ssd_ref as R
    torch.manual_seed(0)
    return R.randomise(M.SSD300(width=width).eval(), 5).to("cuda")


def net_worker(args):
    import torch
    from deeplearningexamples_amd.ssd.infer import SSDDetector
    model = _model()
    eager, graphed = SSDDetector(model, dtype=_dtype(args)), SSDDetector(model, dtype=_dtype(args), graphs=True)
    rows = []
    for b in BATCHES:
        images = torch.randn((b, 3, 300, 300), generator=torch.Generator().manual_seed(2)).to("cuda")
        legs = {"network_eager": lambda: eager.head_outputs(images), "network_graph": lambda: graphed.head_outputs(images),
                "detect_eager": lambda: eager.detect(images), "detect_graph": lambda: graphed.detect(images)}
        for fn in legs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(t.float()).all()) for t in eager.head_outputs(images))
        same = all(torch.equal(a, c) for a, c in zip(eager.detect(images), graphed.detect(images)))
        row = dict(dtype=args.amp_dtype, batch=b, reps=args.reps, finite=finite, graph_equals_eager=same,
                   detections=eager.detect(images)[3].tolist())
        for k, v in timed(legs, args.reps).items():
            row[k] = summarise(v)
            row[k]["img_per_s"] = b * 1000.0 / row[k]["avg_ms"]
        row["post_share_eager_pct"] = 100.0 * (row["detect_eager"]["median_ms"] - row["network_eager"]["median_ms"]) / row["detect_eager"]["median_ms"]
        row["post_share_graph_pct"] = 100.0 * (row["detect_graph"]["median_ms"] - row["network_graph"]["median_ms"]) / row["detect_graph"]["median_ms"]
        rows.append(row)
        del images
    print("RESULT " + json.dumps(rows), flush=True)


def post_worker(args):
    import numpy as np
    import torch
    from deeplearningexamples_amd import functional as F
    from deeplearningexamples_amd.ssd import model as M
    from tests import _ssd_ref as R
    d, labels, n = M.dboxes300_coco(), 81, 32
    parts = [R.case_inputs(d("xywh").numpy(), 2, labels, R.FULL_SEED + i, big_class=True) for i in range(n // 2)]
    ploc = torch.from_numpy(np.concatenate([p[0] for p in parts])).to(_dtype(args))
    plabel = torch.from_numpy(np.concatenate([p[1] for p in parts])).to(_dtype(args))
    heads, geom, start = [], [], 0
    for fs, nd in zip(d.feat_size, d.num_defaults):               # the NHWC head tensors, by the reference's reshape run backwards
        nb = nd * fs * fs
        t = torch.cat((ploc[:, :, start:start + nb].reshape(n, 4 * nd, fs, fs), plabel[:, :, start:start + nb].reshape(n, labels * nd, fs, fs)), 1)
        pitch = (t.shape[1] + 7) // 8 * 8
        t = torch.nn.functional.pad(t.permute(0, 2, 3, 1), (0, pitch - t.shape[1]))
        heads.append(t.contiguous().to("cuda"))
        geom.append((nd, 0, 4 * nd))
        start += nb
    dx = d("xywh").to("cuda").contiguous()
    ploc32, plabel32 = ploc.float().to("cuda"), plabel.float().to("cuda")
    keep = {}

    def kernels():
        boxes, probs = F.ssd_decode(heads, geom, dx, labels, d.scale_xy, d.scale_wh)
        keep["boxes"], keep["probs"] = boxes, probs
        keep["det"] = F.ssd_select(boxes, *F.ssd_nms(boxes, probs, criteria=0.5, threshold=0.05, max_num=200), max_output=200)

    def nms_select():
        keep["det2"] = F.ssd_select(keep["boxes"], *F.ssd_nms(keep["boxes"], keep["probs"], criteria=0.5, threshold=0.05, max_num=200), max_output=200)

    def loop():
        keep["loop_decode"] = R.decode_ref(ploc32, plabel32, dx)          # timed; the sweep below runs on the kernel's own fp32 decode
        keep["loop"] = [R.detect_ref(keep["boxes"][i], keep["probs"][i], 0.5, 200)[:3] for i in range(n)]

    for _ in range(3):
        kernels()
        nms_select()
    loop()
    torch.cuda.synchronize()
    det_boxes, det_label, det_score, det_idx, det_count = (t.cpu() for t in keep["det"])
    same = all(int(det_count[i]) == len(idx) and det_idx[i, :len(idx)].tolist() == idx.tolist() and det_label[i, :len(idx)].tolist() == lab.tolist()
               for i, (idx, lab, _) in enumerate(keep["loop"]))
    ms = timed({"kernels": kernels, "nms_select": nms_select}, args.reps)
    ms.update(timed({"loop": loop}, 3))
    row = dict(dtype=args.amp_dtype, batch=n, reps=args.reps, same_detections_as_loop=same, detections=det_count.tolist(),
               candidates_per_image=[int(v) for v in (keep["probs"][:, 1:] > 0.05).sum((1, 2)).tolist()])
    for k, v in ms.items():
        row[k] = summarise(v)
    row["loop_over_kernels"] = row["loop"]["median_ms"] / row["kernels"]["median_ms"]
    print("RESULT " + json.dumps([row]), flush=True)


def heads_worker(args):
    import torch
    from deeplearningexamples_amd.ssd.infer import SSDDetector
    model = _model()
    dets = {"pad8": SSDDetector(model, dtype=_dtype(args), head_pad=8), "pad64": SSDDetector(model, dtype=_dtype(args), head_pad=64)}
    oc, sizes = model.feature_extractor.out_channels, (38, 19, 10, 5, 3, 1)
    rows = []
    for b in BATCHES:
        g = torch.Generator(device="cuda").manual_seed(b)
        feeds = [torch.randn((b, fs, fs, c), generator=g, device="cuda").to(_dtype(args)) for fs, c in zip(sizes, oc)]
        legs = {k: (lambda det=det: [det._run(u, f) for u, f in zip(det.heads, feeds)]) for k, det in dets.items()}
        for fn in legs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        a, c = legs["pad8"](), legs["pad64"]()
        diff = max(float((x[..., :340].float() - y[..., :340].float()).abs().max()) for x, y in zip(a, c))
        row = dict(dtype=args.amp_dtype, batch=b, reps=args.reps, pitches_pad8=[int(t.shape[3]) for t in a], pitches_pad64=[int(t.shape[3]) for t in c],
                   max_abs_diff_first_340_channels=diff)
        for k, v in timed(legs, args.reps).items():
            row[k] = summarise(v)
        row["pad64_over_pad8"] = row["pad64"]["median_ms"] / row["pad8"]["median_ms"]
        rows.append(row)
    print("RESULT " + json.dumps(rows), flush=True)


def tables(res):
    lines = ["| dtype | batch | network eager ms | network graph ms | detect eager ms | detect graph ms | detect graph img/s | post share (graph) % |",
             "|---|---|---|---|---|---|---|---|"]
    for r in res["net"]:
        lines.append("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.0f | %.1f |" % (
            r["dtype"], r["batch"], r["network_eager"]["median_ms"], r["network_graph"]["median_ms"], r["detect_eager"]["median_ms"],
            r["detect_graph"]["median_ms"], r["detect_graph"]["img_per_s"], r["post_share_graph_pct"]))
    lines += ["", "| dtype | batch | decode + nms + select ms | nms + select ms | python loop ms | loop / kernels | same detections |", "|---|---|---|---|---|---|---|"]
    for r in res["post"]:
        lines.append("| %s | %d | %.4f | %.4f | %.1f | %.0f | %s |" % (r["dtype"], r["batch"], r["kernels"]["median_ms"], r["nms_select"]["median_ms"],
                                                                 r["loop"]["median_ms"], r["loop_over_kernels"], r["same_detections_as_loop"]))
    lines += ["", "| dtype | batch | six heads, pad 8 ms | pad 64 ms | pad 64 / pad 8 | spread % (8, 64) |", "|---|---|---|---|---|---|"]
    for r in res["heads"]:
        lines.append("| %s | %d | %.4f | %.4f | %.3f | %.1f, %.1f |" % (r["dtype"], r["batch"], r["pad8"]["median_ms"], r["pad64"]["median_ms"],
                                                                  r["pad64_over_pad8"], r["pad8"]["spread_pct"], r["pad64"]["spread_pct"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", default=20, type=int)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--groups", default="net,post,heads")
    ap.add_argument("--timeout", default=240, type=int, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssd_infer_perf.json"))
    ap.add_argument("--worker", default=None, choices=["net", "post", "heads"], help=argparse.SUPPRESS)
    ap.add_argument("--amp-dtype", default="fp16", choices=["bf16", "fp16"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return {"net": net_worker, "post": post_worker, "heads": heads_worker}[args.worker](args)
    res, stopped = {"net": [], "post": [], "heads": []}, None
    for kind, dt in [(k, dt) for k in args.groups.split(",") for dt in args.dtypes.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", kind, "--amp-dtype", dt,
               "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not out:
            stopped = dict(job=[kind, dt], returncode=r.returncode, stderr=r.stderr[-2000:])
            print("%s %s: child ended with status %d; the run stops here\n%s" % (kind, dt, r.returncode, r.stderr[-2000:]), flush=True)
            break
        res[kind].extend(json.loads(out[-1][len("RESULT "):]))
        print("%s %s done" % (kind, dt), flush=True)
    print(tables(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(tool="tools/ssd_infer_perf.py", networks=res["net"], post_processing=res["post"], heads=res["heads"], stopped=stopped),
              open(args.out, "w"), indent=1)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
