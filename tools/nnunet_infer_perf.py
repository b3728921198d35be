"""nnU-Net inference timing: the BraTS22 UNet3D of task 11 (six levels, patch 128^3), fp16.

    python tools/nnunet_infer_perf.py [--reps 5] [--no-torch] [--out profiles/nnunet_infer_perf.json]

  convs    each of the 22 convolution launches of one patch batch (N = 1 and 2), exactly as BratsSegmenter issues it (slices of
           the concat buffers, the InstanceNorm table on the operand load, statistic partials), against its MFMA bound
           2 N P Q R 27 C Ko / 2.5 PFLOP/s (dense 16-bit peak of MI355X_MICROARCH), and against the reference's three framework ops
           on the same shape: F.instance_norm in fp32 on the 16-bit input, the cast, F.conv3d (channels_last_3d) and F.relu.
  patch    logits_patch at N = 1 and 2, eager launches and graph replay.
  volume   segment of a [5, 144, 176, 144] volume (a typical cropped BraTS case; 8 windows at overlap 0.5), batches of 2 windows,
           eager and graph replay.

Every leg: three warm-up calls, then `reps` windows of `inner` back-to-back calls between two device events; legs that are compared
are interleaved inside every repetition.  Reported: median / min / max ms per call and the spread (max - min) / median.  The file is
rewritten after every row, so a run that is cut short leaves what it measured.  Weights are random values generated on the
device (timings do not depend on them); a torch leg that fails or exceeds --torch-budget seconds in total is recorded as such.
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

from deeplearningexamples_amd import functional as F                                   # noqa: E402
from deeplearningexamples_amd.nnunet import model as M                                 # noqa: E402
from deeplearningexamples_amd.nnunet.infer import BratsSegmenter                       # noqa: E402

PEAK_16BIT_FLOPS = 2.5e15
PATCH = (128, 128, 128)
VOLUME = (5, 144, 176, 144)


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def interleaved(legs, inner, reps):
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(window(fn, inner))
    return {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), spread=(max(v) - min(v)) / statistics.median(v))
            for k, v in ms.items()}


def device_state(levels, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, shape in M.state_shapes(levels).items():
        if len(shape) == 5:
            out[name] = torch.randn(shape, generator=g, device=dev) * (2.0 / (shape[1] * 27)) ** 0.5
        elif name.endswith("norm.weight"):
            out[name] = 1.0 + 0.1 * torch.randn(shape, generator=g, device=dev)
        else:
            out[name] = 0.1 * torch.randn(shape, generator=g, device=dev)
    return out


def torch_composition(kw, gamma, beta):
    """The reference's ConvLayer on this launch's input slice, as framework ops; returns a callable."""
    x = kw["x"][..., kw["x_off"]:kw["x_off"] + kw["C_in"]].permute(0, 4, 1, 2, 3)            # NCDHW view, channels-last memory
    if x.shape[1] == M.STEM_CHANNELS:
        x = x[:, :M.IN_CHANNELS]
    w = kw["weight"][..., :x.shape[1]].permute(0, 4, 1, 2, 3)                                # [Ko, C, 3, 3, 3], channels-last memory
    x = x.contiguous(memory_format=torch.channels_last_3d)
    w = w.contiguous(memory_format=torch.channels_last_3d)
    stride, normed = kw["stride"], kw["scale"] is not None

    def run():
        h = x
        if normed:
            h = torch.nn.functional.instance_norm(h.float(), weight=gamma, bias=beta, eps=M.EPS)
            if kw["relu_in"]:
                h = torch.relu(h)
            h = h.to(x.dtype)
        y = torch.nn.functional.conv3d(h, w, stride=stride, padding=1)
        return torch.relu(y) if kw["relu_out"] else y
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-budget", type=float, default=600.0, help="seconds of wall time for all torch legs together")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnunet_infer_perf.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    dtype = torch.float16
    result = dict(tool="tools/nnunet_infer_perf.py", device=torch.cuda.get_device_name(0), dtype="fp16", patch=list(PATCH), volume=list(VOLUME),
                  peak_16bit_flops=PEAK_16BIT_FLOPS, reps=a.reps, convs=[], patch_latency=[], volume_latency=[], torch_legs=[])

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)

    sd = device_state(6, dev)
    seg = {g: BratsSegmenter(sd, dtype, graphs=g, patch_size=PATCH, val_batch_size=2) for g in (False, True)}
    plans = {}
    for N in (1, 2):
        x = torch.randn((N, 5) + PATCH, device=dev)
        assert torch.equal(seg[True].logits_patch(x), seg[False].logits_patch(x))
        res = interleaved({"eager": lambda: seg[False].logits_patch(x), "graph": lambda: seg[True].logits_patch(x)}, 3, a.reps)
        result["patch_latency"].append(dict(N=N, **res))
        print(json.dumps(result["patch_latency"][-1]), flush=True)
        save()
        plans[N] = seg[False]._plan(N, *PATCH)
        total_flops = 0.0
        for i, (kw, (key, norm, _, _, _)) in enumerate(zip([k for kind, k in plans[N]["ops"] if kind == "conv"], seg[False].convs)):
            n, d, h, w_, _ = kw["x"].shape
            p, q, r = kw["y"].shape[1:4]
            flops = 2.0 * n * p * q * r * 27 * kw["C_in"] * kw["weight"].shape[0]
            total_flops += flops
            inner = 3 if flops > 2e11 else 10
            t = interleaved({"dle": lambda: F.conv3d_in_fwd(**kw)}, inner, a.reps)["dle"]
            row = dict(index=i, name=key, N=N, input=[d, h, w_], C=kw["C_in"], Ko=int(kw["weight"].shape[0]), stride=kw["stride"], flops=flops,
                       mfma_bound_ms=flops / PEAK_16BIT_FLOPS * 1e3, dle=t, dle_over_mfma_bound=t["ms_median"] / (flops / PEAK_16BIT_FLOPS * 1e3),
                       dle_tflops=flops / (t["ms_median"] * 1e-3) / 1e12)
            result["convs"].append(row)
            print(json.dumps(row), flush=True)
            save()
        result["patch_latency"][-1]["conv_flops"] = total_flops
    vol = torch.randn(VOLUME, device=dev)
    assert torch.equal(seg[True].segment(vol, overlap=0.5), seg[False].segment(vol, overlap=0.5))
    res = interleaved({"eager": lambda: seg[False].segment(vol, overlap=0.5), "graph": lambda: seg[True].segment(vol, overlap=0.5)}, 1, a.reps)
    result["volume_latency"].append(dict(overlap=0.5, blend="constant", windows=len(seg[False]._geometry(VOLUME[1:], 0.5, "constant")["starts"]),
                                         window_batch=2, **res))
    print(json.dumps(result["volume_latency"][-1]), flush=True)
    save()

    if not a.no_torch:
        t0 = time.time()
        for N in (1, 2):
            convs = [k for kind, k in plans[N]["ops"] if kind == "conv"]
            for i, (kw, (key, norm, _, _, _)) in enumerate(zip(convs, seg[False].convs)):
                row = dict(index=i, name=key, N=N)
                if time.time() - t0 > a.torch_budget:
                    row["skipped"] = "the torch legs' time budget of %g s was used up" % a.torch_budget
                else:
                    try:
                        gamma, beta = seg[False].norm[norm] if norm is not None else (None, None)
                        fn = torch_composition(kw, gamma, beta)
                        flops = result["convs"][(N - 1) * len(convs) + i]["flops"]
                        row["torch"] = interleaved({"torch": fn}, 3 if flops > 2e11 else 10, a.reps)["torch"]
                        row["torch_over_dle"] = row["torch"]["ms_median"] / result["convs"][(N - 1) * len(convs) + i]["dle"]["ms_median"]
                    except Exception as e:                                      # recorded, not hidden: the leg is a comparison only
                        row["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
                result["torch_legs"].append(row)
                print(json.dumps(row), flush=True)
                save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
