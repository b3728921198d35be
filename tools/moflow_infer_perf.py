"""MoFlow generation timing at the ZINC250k sizes (N 40, T 10; bond n_squeeze 20, hidden [512, 512], 10 flows; atom 38 flows, gnn
[256], lin [512, 64]), fp16 and bf16, untrained seeded weights (timing does not depend on the values).

    python tools/moflow_infer_perf.py [--reps 5] [--batches 1,8,64,512] [--out profiles/moflow_infer_perf.json]

Per dtype:
  kernels   dle_mf_couple_fwd, dle_mf_bond_decide_fwd and dle_mf_atom_reverse_fwd at batch 512, each against its bound -- the larger
            of (bytes the algorithm needs) / 6.29 TB/s (the measured copy rate) and (MFMA flops) / 2517 TFLOP/s -- and against the
            torch composition of the same step on the GPU (MoFlowModel's modules under autocast: the third Conv2d + the coupling's
            elementwise tail + ActNorm; the symmetrise / softmax / floor tail; GlowOnGraph.reverse);
  reverse   MoFlowGenerator.reverse eager and graph-replayed, and MoFlowModel.reverse under autocast on the GPU, per batch size.
Every leg of a group is timed in ONE process, interleaved, a pair of events around `inner` back-to-back calls after three warm-up
calls; reported: median / min / max ms per call and the spread.  Nothing here is gated.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearningexamples_amd import functional as F                                   # noqa: E402
from deeplearningexamples_amd.moflow.config import ZINC250K_CONFIG                      # noqa: E402
from deeplearningexamples_amd.moflow.infer import MoFlowGenerator                       # noqa: E402
from deeplearningexamples_amd.moflow.model import MoFlowModel                           # noqa: E402

HBM, MFMA = 6.29e12, 2517e12


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


def seeded_model():
    torch.manual_seed(0)
    m = MoFlowModel(ZINC250K_CONFIG).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, t in m.state_dict().items():
            if name.endswith("running_var") or name.endswith("actnorm.scale"):
                t.copy_(torch.rand(t.shape, generator=g) * 0.5 + 0.75)
            elif name.endswith("running_mean") or name.endswith("actnorm.loc"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moflow_infer_perf.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = ZINC250K_CONFIG
    n, t, fold, z_dim = cfg.max_num_nodes, cfg.num_node_features, cfg.model_config.bond_config.n_squeeze, cfg.z_dim
    model = seeded_model()
    gpu_model = MoFlowModel(cfg).eval()
    gpu_model.load_state_dict(model.state_dict())
    gpu_model = gpu_model.to(dev)
    batches = [int(v) for v in a.batches.split(",")]
    out = {"config": "zinc250k", "hbm_bytes_per_s": HBM, "mfma_flops_per_s": MFMA, "kernels": [], "reverse": []}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        eager, graphed = MoFlowGenerator(model, dtype), MoFlowGenerator(model, dtype, graphs=True)
        g = torch.Generator().manual_seed(2)

        # ---- kernels at batch 512
        b = 512
        z = (torch.randn(b, z_dim, generator=g) * 0.6).to(dev)
        f = eager.bond[-1]
        p, m2, k = eager.positions, f["w3"].shape[0], f["w3"].shape[1]
        h2 = torch.rand(b, k, generator=g).to(dev, dtype)
        state = torch.randn(b, p, m2 // p, generator=g).to(dev)
        flow = gpu_model.bond_model.blocks[0].flows[-1]
        y4 = torch.randn(b, 1600, 2, 2, generator=g).to(dev)
        h2c = torch.rand(b, 512, 2, 2, generator=g).to(dev)

        def couple_torch():
            with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                ya, yb = y4.chunk(2, 1)
                s, tt = flow.coupling.layers[6](h2c).chunk(2, 1)
                return flow.actnorm.reverse(torch.cat([ya, yb * (1 + torch.exp(-s)) - tt], 1))

        def decide_torch():
            with torch.no_grad():
                return gpu_model.discretise(y4.reshape(b, 4, n, n))

        mask = F.mf_bond_decide_fwd(state, n, fold, False)[0]
        adj = torch.stack([((mask >> e) & 1).float() for e in range(4)], 1)

        def atom_torch():
            with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                return gpu_model.atom_reverse(adj, z)

        legs = {
            "couple": lambda: F.mf_couple_fwd(h2, f["w3"], f["b3"], f["scale"], f["loc"], state, p, f["swap"], img_half=0),
            "couple_torch": couple_torch,
            "decide": lambda: F.mf_bond_decide_fwd(state, n, fold, False, want_adj=True),
            "decide_torch": decide_torch,
            "atom": lambda: F.mf_atom_reverse_fwd(z[:, :n * t], mask, eager.w16, eager.p32, n, t, eager.hidden_gnn, eager.hidden_lin, 1, False),
            "atom_torch": atom_torch,
        }
        res = interleaved(legs, 5, a.reps)
        a_cfg = cfg.model_config.atom_config
        atom_flops = 2.0 * b * a_cfg.n_flow * ((4 * t + 4) * 256 + 256 * 512 + 512 * 64 + 64 * 2 * t)
        work = {"couple": (2.0 * m2 * k + 2.0 * b * k + 4.0 * 2 * b * m2 + 2.0 * b * m2 // 2, 2.0 * b * m2 * k),
                "decide": (4.0 * b * 4 * n * n * 2 + 2.0 * b * n * n, 0.0),
                "atom": (2.0 * eager.w16.numel() + b * (8.0 * n * t + n * n * a_cfg.n_flow / n), atom_flops)}
        for kname, (by, fl) in work.items():
            bound = max(by / HBM, fl / MFMA) * 1e3
            r = dict(res[kname], kernel=kname, dtype=name, batch=b, bytes=by, mfma_flops=fl, bound_ms=bound,
                     bound_by="bytes" if by / HBM >= fl / MFMA else "mfma", times_bound=res[kname]["ms_median"] / bound,
                     torch_ms_median=res[kname + "_torch"]["ms_median"], torch_spread=res[kname + "_torch"]["spread"],
                     speedup_over_torch=res[kname + "_torch"]["ms_median"] / res[kname]["ms_median"])
            out["kernels"].append(r)
            print("%s %-7s %8.4f ms  bound %8.4f ms (%s, x%.1f)  torch %8.4f ms (x%.1f)" %
                  (name, kname, r["ms_median"], bound, r["bound_by"], r["times_bound"], r["torch_ms_median"], r["speedup_over_torch"]))

        # ---- reverse per batch size
        for b in batches:
            z = (torch.randn(b, z_dim, generator=g) * 0.6).to(dev)

            def baseline():
                with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                    return gpu_model.reverse(z)
            res = interleaved({"eager": lambda: eager.reverse(z), "graph": lambda: graphed.reverse(z), "torch_autocast": baseline}, 3, a.reps)
            row = dict(dtype=name, batch=b, **{k + "_" + q: v[q] for k, v in res.items() for q in ("ms_median", "ms_min", "ms_max", "spread")})
            row["molecules_per_s_graph"] = b / (res["graph"]["ms_median"] * 1e-3)
            row["speedup_eager"] = res["torch_autocast"]["ms_median"] / res["eager"]["ms_median"]
            row["speedup_graph"] = res["torch_autocast"]["ms_median"] / res["graph"]["ms_median"]
            out["reverse"].append(row)
            print("%s batch %4d  eager %8.3f ms  graph %8.3f ms  torch autocast %8.3f ms  (x%.1f / x%.1f)" %
                  (name, b, res["eager"]["ms_median"], res["graph"]["ms_median"], res["torch_autocast"]["ms_median"], row["speedup_eager"],
                   row["speedup_graph"]))
        del eager, graphed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
