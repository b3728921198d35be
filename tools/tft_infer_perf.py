"""TFT inference on the MI355X: every kernel of csrc/tft.hip against a torch composition of the same operations on the same device
and type, the one-launch LSTM against T launches of dle_t2_lstm_gemm_fwd, and TFTForecaster.forecast (eager and graph replay)
against the host model run with torch operators in the same 16-bit type, at batch 1, 64 and 1024 of the electricity configuration
(T = 192, encoder 168).  Writes profiles/tft_infer_perf.json.

    python tools/tft_infer_perf.py [--out profiles/tft_infer_perf.json] [--batches 1 64 1024]

Timing: device events around `iters` back-to-back calls after `warmup` calls, the median of `repeats` such windows; every
window is at least tens of milliseconds.  No GPU, no number: the script fails without a device.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeplearningexamples_amd import _cabi as C                     # noqa: E402
from deeplearningexamples_amd import functional as F                # noqa: E402
from deeplearningexamples_amd.tft import model as TM                # noqa: E402
from deeplearningexamples_amd.tft.infer import TFTForecaster        # noqa: E402

H = 128


def timed(fn, warmup=5, iters=50, repeats=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)
    out.sort()
    return {"us": out[len(out) // 2], "us_min": out[0], "us_max": out[-1]}


def kernels(dtype, rows_list, dev):
    res = []
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    grn_mod = TM.GRN(H, H, context_hidden_size=H).to(dev, dtype).eval()
    pack = F.tft_grn_pack({k: v for k, v in grn_mod.state_dict().items()}, dtype, dev)
    for B in rows_list:
        T, enc = 192, 168
        rows = B * T
        x, ctx = r(B, T, H).to(dev, dtype), r(B, H).to(dev, dtype)
        with torch.no_grad():
            a = timed(lambda: F.tft_grn_fwd(x.view(rows, H), pack, ctx=ctx, rows_per_ctx=T))
            b = timed(lambda: grn_mod(x, ctx))
        res.append({"kernel": "dle_tft_grn_fwd", "what": "enrichment GRN, %d rows" % rows, "batch": B, "fused": a, "torch": b, "ratio": a["us"] / b["us"]})
        # VSN over 4 continuous variables (history)
        cfg = TM.ElectricityConfig()
        vsn_mod = TM.VariableSelectionNetwork(cfg, 4).to(dev, dtype).eval()
        vec, bias = r(4, H), 0.1 * r(4, H)
        vp = F.tft_vsn_pack({k: v.float() for k, v in vsn_mod.state_dict().items()}, vec, bias, dtype, dev)
        vals = r(B, T, 4).to(dev)
        vec_d, bias_d = vec.to(dev, dtype), bias.to(dev, dtype)
        with torch.no_grad():
            a = timed(lambda: F.tft_vsn_fwd([vals], vp, dtype, enc, ctx=ctx))
            b = timed(lambda: vsn_mod(vals[:, :enc].to(dtype).unsqueeze(-1) * vec_d + bias_d, ctx))
        res.append({"kernel": "dle_tft_vsn_fwd", "what": "history VSN, F = 4, %d rows" % (B * enc), "batch": B, "fused": a, "torch": b,
                    "ratio": a["us"] / b["us"]})
        # LSTM over 168 steps
        lstm = torch.nn.LSTM(H, H, batch_first=True).to(dev, dtype).eval()
        feat = r(B, enc, H).to(dev, dtype)
        h0, c0 = r(B, H).to(dev, dtype), r(B, H).to(dev, dtype)
        w_ih, w_hh = lstm.weight_ih_l0.detach().contiguous(), lstm.weight_hh_l0.detach().contiguous()
        bsum = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().float().contiguous()

        def fused():
            xp = F.gemm(feat.view(B * enc, H), w_ih, B * enc, 4 * H, H, True, True, out_dtype=torch.float32, bias=bsum).view(B, enc, 4 * H)
            return F.tft_lstm_fwd(xp, w_hh, h0, c0)

        xp16 = F.gemm(feat.view(B * enc, H), w_ih, B * enc, 4 * H, H, True, True, bias=bsum).view(B, enc, 4 * H).transpose(0, 1).contiguous()
        gates = torch.empty(B, 4 * H, dtype=dtype, device=dev)
        hbuf = [h0.clone(), torch.empty_like(h0)]
        cbuf = [c0.float().contiguous(), torch.empty(B, H, device=dev)]

        def per_step():
            for t in range(enc):
                C.call("dle_t2_lstm_gemm_fwd", C.ptr(hbuf[t & 1]), H, C.ptr(w_hh), H, 0, C.ptr(xp16[t]), C.ptr(cbuf[t & 1]), C.ptr(cbuf[(t + 1) & 1]),
                       C.ptr(gates), 4 * H, C.ptr(hbuf[(t + 1) & 1]), H, 0, 0, 0, 0, 0, 0, 1.0, B, H, H, C.dt(dtype), C.stream())

        with torch.no_grad():
            a = timed(fused, iters=20)
            b = timed(lambda: lstm(feat, (h0.unsqueeze(0), c0.unsqueeze(0))), iters=20)
            try:
                c = timed(per_step, iters=5)
            except (ValueError, C.DleError) as err:                  # outside that kernel's envelope: recorded, not hidden
                c = {"us": float("nan"), "not_measured": str(err)}
        res.append({"kernel": "dle_gemm + dle_tft_lstm_fwd", "what": "history encoder, 168 steps", "batch": B, "fused": a, "torch": b,
                    "per_step_launches": c, "ratio": a["us"] / b["us"], "ratio_per_step": a["us"] / c["us"]})
        a1 = timed(lambda: F.tft_lstm_fwd(F.gemm(feat.view(B * enc, H), w_ih, B * enc, 4 * H, H, True, True, out_dtype=torch.float32,
                                                 bias=bsum).view(B, enc, 4 * H)[:, :1], w_hh, h0, c0), iters=20)
        res[-1]["us_per_step"] = (a["us"] - a1["us"]) / (enc - 1)
        # attention of the 24 decoder positions
        att = TM.InterpretableMultiHeadAttention(cfg).to(dev, dtype).eval()
        w_qkv, w_o = att.qkv_linears.weight.detach().contiguous(), att.out_proj.weight.detach().contiguous()
        xin = r(B, T, H).to(dev, dtype)
        qkv = F.gemm(xin.view(B * T, H), w_qkv, B * T, 288, H, True, True)
        with torch.no_grad():
            a = timed(lambda: F.tft_attention_fwd(qkv, w_o, B, T, enc))

            def torch_attn():
                q, k, v = qkv.view(B, T, 288).split((128, 128, 32), dim=-1)
                q, k = q.view(B, T, 4, 32).transpose(1, 2), k.view(B, T, 4, 32).transpose(1, 2)
                p = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * att.scale + att._mask, dim=3)
                return torch.nn.functional.linear(torch.matmul(p, v.unsqueeze(1)).mean(1), w_o)[:, enc:]
            b = timed(torch_attn)
        res.append({"kernel": "dle_tft_attention_fwd", "what": "24 of 192 positions (torch: all 192, as the reference)", "batch": B, "fused": a,
                    "torch": b, "ratio": a["us"] / b["us"]})
    return res


def forecasts(dtype, batches, dev):
    cfg = TM.ElectricityConfig()
    torch.manual_seed(0)
    model = TM.TemporalFusionTransformer(cfg).eval()
    host = TM.TemporalFusionTransformer(cfg).to(dev, dtype).eval()
    host.load_state_dict(model.state_dict())
    eager, graphed = TFTForecaster(model, dtype=dtype), TFTForecaster(model, dtype=dtype, graphs=True)
    res = []
    for B in batches:
        T = cfg.example_length
        batch = {"s_cat": torch.randint(0, 369, (B, 1, 1), device=dev).expand(B, T, 1).contiguous(), "s_cont": None, "o_cont": None,
                 "k_cont": torch.randn(B, T, 3, device=dev), "target": torch.randn(B, T, 1, device=dev)}
        b16 = {k: (v.to(dtype) if v is not None and v.is_floating_point() else v) for k, v in batch.items()}
        iters = 20 if B <= 64 else 5
        with torch.no_grad():
            a = timed(lambda: eager.forecast(batch), iters=iters)
            g = timed(lambda: graphed.forecast(batch), iters=iters)
            h = timed(lambda: host(b16), iters=iters)
            names = []
            real = C.call
            C.call = lambda nm, *args: (names.append(nm), real(nm, *args))[1]
            try:
                eager.forecast(batch)
            finally:
                C.call = real
        res.append({"batch": B, "launches": len(names), "forecast_eager": a, "forecast_graph": g, "host_model_torch": h,
                    "eager_over_torch": a["us"] / h["us"], "graph_over_torch": g["us"] / h["us"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tft_infer_perf.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tft_infer_perf: no GPU, no measurement")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "method": "device events around back-to-back calls, median of 5 windows", "dtypes": {}}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        out["dtypes"][name] = {"kernels": kernels(dtype, args.batches, dev), "forecast": forecasts(dtype, args.batches, dev)}
        for k in out["dtypes"][name]["kernels"]:
            print(name, k["kernel"], k["what"], "B", k["batch"], "fused %.1f us" % k["fused"]["us"], "torch %.1f us" % k["torch"]["us"],
                  "ratio %.3f" % k["ratio"], ("per-step launches %.1f us, %.3f us/step" % (k["per_step_launches"]["us"], k["us_per_step"]))
                  if "per_step_launches" in k else "", flush=True)
        for f in out["dtypes"][name]["forecast"]:
            print(name, "forecast B", f["batch"], "launches", f["launches"], "eager %.1f us" % f["forecast_eager"]["us"],
                  "graph %.1f us" % f["forecast_graph"]["us"], "torch host model %.1f us" % f["host_model_torch"]["us"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
