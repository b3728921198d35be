"""Jasper 10x5dr inference timing on the MI355X: the dense packed conv1d kernel per distinct layer shape against the one earlier
path that computes the same thing, and the whole recognizer.

    python tools/jasper_infer_perf.py [--reps 12] [--out profiles/jasper_infer_perf.json]

Layers.  Per distinct layer shape of the 10x5dr network -- Conv1 (64 -> 256, k 11, stride 2), the first and the other sub-blocks
of B1 .. B5, Conv2 (768 -> 896, k 29, dilation 2), Conv3 (896 -> 1024, k 1) -- at 1 x 1,686 and 16 x 1,686 input frames (843 rows
per utterance behind the stride-2 Conv1), bf16:
  `new`         one F.conv1d_bn_packed_fwd launch (with residual for the shapes that close a block, ReLU always);
  `comparator`  dle_conv2d_fwd_affine with R = 1, S = ksize over ONE zero-padded batch [B, 1, T + 2 halo, C] (pad 0, so that the
                padding is in the tensor and the output is [B, 1, T, Ko]), the only path of the parent commit that computes the same
                sums; dilation-1, stride-1 shapes only, and only where its envelope admits the shape (otherwise the reason it
                gave is recorded).  Its output is compared with the new kernel's once, before anything is timed.
Both are measured in one process, alternated sample by sample (new, comparator, new, comparator, ...), same operands, after 3
warm-up launches each.  A sample is LAUNCHES launches back to back between two device events, divided by LAUNCHES.  Reported per
alternative: median, minimum and `spread_pct` (the median of its even samples against the median of its odd samples: the spread
of repeated runs on this box); `spread_pct_max` at the top is the largest over all rows.  `new_over_comparator` is the ratio of
the medians; `loses` is true where it exceeds 1.05.  From the shapes: mfma_flops = 2 rows ksize C Ko, t_mfma_us at the 2500
TFLOP/s of bench.py's roofline, and `frac_of_mfma_bound` = t_mfma / median time.

Recognizer.  Seeded random weights (Xavier-uniform, identity BatchNorm statistics), seeded log-mel-like features, fp16, batch 1 and
16 at 2 s, 7 s and 16.7 s (200, 700 and 1,670 frames + 16 lead frames): one decode() call between host timestamps, ending in the
call's own device-to-host read; median of the calls after 3 warm-ups.  `residual_share`: one more call under _cabi.KernelTimer
(an event pair around every launch): the time inside the 55 dle_conv2d_fwd_affine launches over the time inside all launches.
Nothing here fixes a speed in advance.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0
# name, C, Ko, ksize, stride, dilation, residual
LAYER_SHAPES = [("conv1", 64, 256, 11, 2, 1, False), ("b1", 256, 256, 11, 1, 1, True),
                ("b2_first", 256, 384, 13, 1, 1, False), ("b2", 384, 384, 13, 1, 1, True),
                ("b3_first", 384, 512, 17, 1, 1, False), ("b3", 512, 512, 17, 1, 1, True),
                ("b4_first", 512, 640, 21, 1, 1, False), ("b4", 640, 640, 21, 1, 1, True),
                ("b5_first", 640, 768, 25, 1, 1, False), ("b5", 768, 768, 25, 1, 1, True),
                ("conv2", 768, 896, 29, 1, 2, False), ("conv3", 896, 1024, 1, 1, 1, False)]
FRAMES, ROWS = 1686, 843
LAUNCHES = 5
DURATIONS = ((2.0, 200), (7.0, 700), (16.7, 1670))


def summarise(ms):
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2])
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), spread_pct=100.0 * abs(even - odd) / min(even, odd))


def sample(call):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        call()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


def layer_leg(reps):
    import torch
    from deeplearningexamples_amd import functional as F
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    for seqs in (1, 16):
        for name, c, ko, ks, stride, dil, use_res in LAYER_SHAPES:
            t_in = ROWS * stride
            cu = lambda l: torch.tensor([0] + torch.tensor(l).cumsum(0).tolist(), dtype=torch.int32, device=dev)
            cu_in, cu_out = cu([t_in] * seqs), cu([ROWS] * seqs)
            rows = seqs * ROWS
            x = torch.randn((seqs * t_in, c), generator=g, device=dev).to(dt)
            w = (torch.randn((ko, ks, c), generator=g, device=dev) * (ks * c) ** -0.5).to(dt)
            sc, sh = torch.rand(ko, generator=g, device=dev) + 0.5, torch.randn(ko, generator=g, device=dev)
            res = torch.randn((rows, ko), generator=g, device=dev).to(dt) if use_res else None
            y = torch.empty((rows, ko), dtype=dt, device=dev)
            new = lambda: F.conv1d_bn_packed_fwd(x, w, sc, sh, cu_in, cu_out, rows, stride=stride, dilation=dil, residual=res,
                                                 relu=True, out=y)
            old, why = None, None
            if stride == 1 and dil == 1:
                halo = ks // 2
                xp = torch.zeros((seqs, 1, ROWS + 2 * halo, c), dtype=dt, device=dev)
                xp[:, 0, halo:halo + ROWS] = x.view(seqs, ROWS, c)
                w4 = w.view(ko, 1, ks, c)
                r4 = res.view(seqs, 1, ROWS, ko) if use_res else None
                y4 = torch.empty((seqs, 1, ROWS, ko), dtype=dt, device=dev)
                old = lambda: F.conv2d_fwd_affine(xp, w4, sc, sh, stride=1, pad=0, residual=r4, relu=True, out=y4)
                try:
                    old()
                    new()
                    torch.cuda.synchronize()
                    diff = float((y4.view(rows, ko).float() - y.float()).abs().max())
                except (ValueError, RuntimeError) as e:
                    old, why = None, str(e).splitlines()[0]
            else:
                why = "stride or dilation 2: outside the comparator's reach"
            for _ in range(3):
                new()
                if old:
                    old()
            ms_new, ms_old = [], []
            for _ in range(reps):
                ms_new.append(sample(new))
                if old:
                    ms_old.append(sample(old))
            r = dict(name=name, seqs=seqs, rows=rows, C=c, Ko=ko, ksize=ks, stride=stride, dilation=dil, residual=use_res,
                     new=summarise(ms_new))
            flops = 2.0 * rows * ks * c * ko
            t_mfma = flops / (MFMA_PEAK_TFLOPS * 1e6)
            r.update(mfma_flops=flops, t_mfma_us=t_mfma, frac_of_mfma_bound=t_mfma / (r["new"]["median_ms"] * 1e3),
                     tflops=flops / (r["new"]["median_ms"] * 1e9))
            if old:
                r["comparator"] = summarise(ms_old)
                r["comparator_frac_of_mfma_bound"] = t_mfma / (r["comparator"]["median_ms"] * 1e3)
                r["max_abs_diff_against_comparator"] = diff
                r["new_over_comparator"] = r["new"]["median_ms"] / r["comparator"]["median_ms"]
                r["loses"] = r["new_over_comparator"] > 1.05
            else:
                r["comparator"] = None
                r["comparator_not_run"] = why
            print(json.dumps(r), flush=True)
            out.append(r)
    return out


def random_state(cfg, seed):
    import torch
    from deeplearningexamples_amd.jasper.model import state_shapes
    g = torch.Generator().manual_seed(seed)
    st = {}
    for k, shape in state_shapes(cfg).items():
        if k.endswith("num_batches_tracked"):
            st[k] = torch.zeros((), dtype=torch.int64)
        elif len(shape) == 3:
            bound = (6.0 / ((shape[0] + shape[1]) * shape[2])) ** 0.5
            st[k] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif k.endswith("running_var") or (k.endswith(".weight") and len(shape) == 1):
            st[k] = torch.ones(shape)
        else:
            st[k] = torch.zeros(shape)
    return st


def network_leg(reps, config):
    import torch
    from deeplearningexamples_amd import _cabi as C
    from deeplearningexamples_amd.jasper.infer import JasperRecognizer
    rec = JasperRecognizer(random_state(config, 3), config, torch.float16)
    g = torch.Generator().manual_seed(4)
    out = []
    for batch in (1, 16):
        for seconds, frames in DURATIONS:
            lens = [frames] * batch
            feats = [(torch.randn((64, frames), generator=g) * 2 - 6) for _ in lens]
            for _ in range(3):
                rec.decode(feats, lens)
            ms = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.time()
                rec.decode(feats, lens)
                ms.append((time.time() - t0) * 1e3)
            row = dict(batch=batch, seconds=seconds, frames=frames, lead=rec.pad_leading, **summarise(ms))
            timer = C.KernelTimer()
            prev = C.set_timer(timer)
            try:
                rec.decode(feats, lens)
            finally:
                C.set_timer(prev)
            by_name = {}
            for a in timer.report():
                by_name[a["name"]] = by_name.get(a["name"], 0.0) + a["ms"]
            row["launch_ms"] = by_name
            row["residual_share"] = by_name.get("dle_conv2d_fwd_affine", 0.0) / sum(by_name.values())
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jasper_infer_perf.json"))
    ap.add_argument("--config", default=None, help="the reference's 10x5dr YAML (default: the same configuration restated here)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    if args.config:
        from deeplearningexamples_amd.utils.state import load_config
        config = json.loads(json.dumps(load_config(args.config)))            # (the YAML's anchors share block dicts)
    else:
        config = config_10x5dr()
    layers = layer_leg(args.reps)
    spreads = [r["new"]["spread_pct"] for r in layers] + [r["comparator"]["spread_pct"] for r in layers if r["comparator"]]
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, launches_per_sample=LAUNCHES,
                  peaks=dict(mfma_tflops=MFMA_PEAK_TFLOPS), spread_pct_max=max(spreads), spread_pct_median=statistics.median(spreads),
                  layers=layers, losing_shapes=[(r["name"], r["seqs"]) for r in layers if r.get("loses")],
                  network=network_leg(max(5, args.reps // 2), config))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def config_10x5dr():
    def blk(f, r, k, s=1, d=1, res=True):
        b = dict(filters=f, repeat=r, kernel_size=[k], stride=[s], dilation=[d], dropout=0.0, residual=res)
        if res:
            b["residual_dense"] = True
        return b
    blocks = [blk(256, 1, 11, s=2, res=False)]
    for f, k in ((256, 11), (384, 13), (512, 17), (640, 21), (768, 25)):
        blocks += [blk(f, 5, k) for _ in range(2)]
    blocks += [blk(896, 1, 29, d=2, res=False), blk(1024, 1, 1, res=False)]
    labels = [" "] + [chr(ord("a") + i) for i in range(26)] + ["'"]
    feats = dict(normalize="per_feature", sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", n_filt=64, n_fft=512,
                 frame_splicing=1, dither=0.00001, pad_align=16)
    return dict(labels=labels, input_val=dict(audio_dataset=dict(sample_rate=16000), filterbank_features=feats),
                jasper=dict(encoder=dict(in_feats=64, activation="relu", use_conv_masks=True, frame_splicing=1, blocks=blocks),
                            decoder=dict(in_feats=1024)))


if __name__ == "__main__":
    main()
