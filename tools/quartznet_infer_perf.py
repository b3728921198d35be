"""QuartzNet 15x5 inference timing on the MI355X: the fused separable kernel per distinct unit shape, and the whole recognizer
packed against padded.

    python tools/quartznet_infer_perf.py [--reps 30] [--out profiles/quartznet_infer_perf.json]

Per distinct unit shape of the 15x5 network -- Conv1 (64 -> 256, k 33, stride 2), the block shapes (256 -> 256 k 33 / 39, 256 -> 512
k 51, 512 -> 512 k 51 / 63 / 75), Conv2 (512 -> 512, k 87, dilation 2) -- at 8 sequences x 835 output rows (16.7 s utterances behind
the stride-2 Conv1), bf16: the time of one F.tcs_conv1d_packed_fwd launch (with residual and ReLU for the block shapes) in BOTH forms of the
kernel's chunk loop, forced with F.tcs_prefetch_mode (plain, prefetch, plain, prefetch: the repeats show the run-to-run spread; same
process, same operands).  Every sample is 20 launches back to back between two device events, divided by 20, after 5 warm-up
launches, so the events and the launch gaps of a 30 - 70 us kernel weigh 1/20 of what they do on a single launch; the operands stay in
L2 / Infinity Cache between launches, as they do between the units of the network.  Reported per form: median, minimum and
`spread_pct` (the median of the even against the odd samples); the top-level figures are those of the form the launcher chooses at
this grid (`chosen`).  What the algorithm needs, computed from the shapes:
    hbm_bytes   x + dw + pw + scale + shift + y (+ residual), each read or written once
    mfma_flops  2 rows C Ko (the pointwise product)
    valu_flops  2 rows C ksize x (Ko / 256 channel blocks: the depthwise is recomputed per block of 256 output channels)
and the bounds those imply with the peak figures of bench.py's roofline (8000 GB/s, 2500 TFLOP/s on MFMA) and the fp32 vector peak
of 157.3 TFLOP/s: t_hbm, t_mfma, t_valu in microseconds.  `bound` names the largest; `frac_of_bound` = that bound / median time.

Whole recognizer: seeded random weights (tests-free: Xavier-uniform weights, identity BatchNorm statistics), seeded log-mel-like
features, batch 1, 8 and 32, fp16.  `fill` 1.0: every utterance 1670 frames (16.7 s); fill 0.5 / 0.25: the lengths are drawn uniformly
so that the MEAN length is that share of the longest (1670 frames).  `packed` = the recognizer on those lengths; `padded` = the same
kernels with every length set to the longest (what a padded batch costs: the comparison tools/bert_infer_perf.py makes).  Latency
= one decode() call between host timestamps, ending in the call's own device-to-host read; median of --reps calls after 3 warm-ups.
No speed threshold is fixed: there is no earlier path to compare with.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS, MFMA_PEAK_TFLOPS, VALU_PEAK_TFLOPS = 8000.0, 2500.0, 157.3
# name, C, Ko, ksize, stride, dilation, residual
UNIT_SHAPES = [("conv1", 64, 256, 33, 2, 1, False), ("b1", 256, 256, 33, 1, 1, True), ("b2", 256, 256, 39, 1, 1, True),
               ("b3_first", 256, 512, 51, 1, 1, False), ("b3", 512, 512, 51, 1, 1, True), ("b4", 512, 512, 63, 1, 1, True),
               ("b5", 512, 512, 75, 1, 1, True), ("conv2", 512, 512, 87, 1, 2, False)]
SEQS, ROWS, LONGEST = 8, 835, 1670
LAUNCHES = 20          # launches per timed sample: one 30 - 70 us launch between two events measures the events as much as the kernel


def summarise(ms):
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2])
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), spread_pct=100.0 * abs(even - odd) / min(even, odd))


def unit_leg(reps):
    import torch
    from deeplearningexamples_amd import functional as F
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    for name, c, ko, ks, stride, dil, use_res in UNIT_SHAPES:
        in_len = ROWS * stride
        lens_in, lens_out = [in_len] * SEQS, [ROWS] * SEQS
        cu = lambda l: torch.tensor([0] + torch.tensor(l).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        cu_in, cu_out = cu(lens_in), cu(lens_out)
        rows = SEQS * ROWS
        x = torch.randn((SEQS * in_len, c), generator=g, device=dev).to(dt)
        dw = (torch.randn((ks, c), generator=g, device=dev) * ks ** -0.5).to(dt)
        pw = (torch.randn((ko, c), generator=g, device=dev) * c ** -0.5).to(dt)
        sc, sh = torch.ones(ko, device=dev), torch.zeros(ko, device=dev)
        res = torch.randn((rows, ko), generator=g, device=dev).to(dt) if use_res else None
        y = torch.empty((rows, ko), dtype=dt, device=dev)
        call = lambda: F.tcs_conv1d_packed_fwd(x, dw, pw, sc, sh, cu_in, cu_out, rows, stride=stride, dilation=dil, residual=res,
                                               relu=True, out=y)
        forms = {}
        for form, mode in (("plain", 0), ("prefetch", 1), ("plain_again", 0), ("prefetch_again", 1)):
            F.tcs_prefetch_mode(mode)
            for _ in range(5):
                call()
            ms = []
            for _ in range(reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(LAUNCHES):
                    call()
                e.record()
                e.synchronize()
                ms.append(s.elapsed_time(e) / LAUNCHES)
            forms[form] = summarise(ms)
        F.tcs_prefetch_mode(2)
        grid = (rows // 64 + SEQS) * ((ko + 255) // 256)
        chosen = "prefetch" if grid <= torch.cuda.get_device_properties(0).multi_processor_count else "plain"
        r = dict(forms[chosen], chosen=chosen, grid=grid, forms=forms)
        nbytes = 2.0 * (x.numel() + dw.numel() + pw.numel() + y.numel() * (2 if use_res else 1)) + 8.0 * ko
        mfma, valu = 2.0 * rows * c * ko, 2.0 * rows * c * ks * ((ko + 255) // 256)
        bounds = dict(t_hbm_us=nbytes / (HBM_PEAK_GBS * 1e3), t_mfma_us=mfma / (MFMA_PEAK_TFLOPS * 1e6), t_valu_us=valu / (VALU_PEAK_TFLOPS * 1e6))
        top = max(bounds, key=bounds.get)
        r.update(name=name, C=c, Ko=ko, ksize=ks, stride=stride, dilation=dil, residual=use_res, rows=rows, hbm_bytes=nbytes,
                 mfma_flops=mfma, valu_flops=valu, bound=top[2:-3], frac_of_bound=bounds[top] / (r["median_ms"] * 1e3), **bounds)
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def random_state(cfg, seed):
    import torch
    from deeplearningexamples_amd.quartznet.model import state_shapes
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
    from deeplearningexamples_amd.quartznet.infer import QuartzNetRecognizer
    rec = QuartzNetRecognizer(random_state(config, 3), config, torch.float16)
    g = torch.Generator().manual_seed(4)
    out = []
    for batch in (1, 8, 32):
        for fill in (1.0, 0.5, 0.25):
            if fill == 1.0:
                lens = [LONGEST] * batch
            else:
                lo = max(2, int((2 * fill - 1) * LONGEST)) if fill > 0.5 else 2
                hi = int(2 * fill * LONGEST) - lo
                lens = [LONGEST] + [int(torch.randint(lo, max(hi, lo + 1), (1,), generator=g)) for _ in range(batch - 1)]
            feats = [(torch.randn((64, LONGEST), generator=g) * 2 - 6) for _ in lens]
            row = dict(batch=batch, fill_target=fill, fill=sum(lens) / (LONGEST * len(lens)))
            for leg, ll in (("packed", lens), ("padded", [LONGEST] * len(lens))):
                for _ in range(3):
                    rec.decode(feats, ll)
                ms = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    rec.decode(feats, ll)
                    ms.append((time.time() - t0) * 1e3)
                row[leg] = summarise(ms)
            row["packed_over_padded"] = row["packed"]["median_ms"] / row["padded"]["median_ms"]
            print(json.dumps(row), flush=True)
            out.append(row)
            if batch == 1:
                break                                                   # one utterance: nothing to pad
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartznet_infer_perf.json"))
    ap.add_argument("--config", default=None, help="the reference's 15x5 YAML (default: the same configuration restated here)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    if args.config:
        from deeplearningexamples_amd.utils.state import load_config
        config = load_config(args.config)
    else:
        config = config_15x5()
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, peaks=dict(hbm_gbs=HBM_PEAK_GBS, mfma_tflops=MFMA_PEAK_TFLOPS,
                                                                                   valu_tflops=VALU_PEAK_TFLOPS),
                  units=unit_leg(args.reps), network=network_leg(max(5, args.reps // 3), config))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def config_15x5():
    blk = lambda f, r, k, s=1, d=1, res=True, sep=True: dict(filters=f, repeat=r, kernel_size=[k], stride=[s], dilation=[d], dropout=0.0,
                                                            residual=res, separable=sep)
    blocks = [blk(256, 1, 33, s=2, res=False)]
    for f, k in ((256, 33), (256, 39), (512, 51), (512, 63), (512, 75)):
        blocks += [blk(f, 5, k) for _ in range(3)]
    blocks += [blk(512, 1, 87, d=2, res=False), blk(1024, 1, 1, res=False, sep=False)]
    labels = [" "] + [chr(ord("a") + i) for i in range(26)] + ["'"]
    feats = dict(normalize="per_feature", sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", n_filt=64, n_fft=512,
                 frame_splicing=1, dither=0.00001, pad_align=16)
    return dict(labels=labels, input_val=dict(audio_dataset=dict(sample_rate=16000), filterbank_features=feats),
                quartznet=dict(encoder=dict(in_feats=64, activation="relu", use_conv_masks=True, frame_splicing=1, blocks=blocks),
                               decoder=dict(in_feats=1024)))


if __name__ == "__main__":
    main()
