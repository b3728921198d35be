"""DLRM inference timing: the Criteo-shape model (26 tables capped at --cap rows, dim 128, the default MLPs), batches of 1, 64, 4096
and 65536, fp16.

    python tools/dlrm_infer_perf.py [--cap 100000] [--reps 9] [--out profiles/dlrm_infer_perf.json]

Per batch size the four legs of DlrmPredictor.predict -- fused / unfused interaction x eager launches / graph replay -- are timed in
ONE process, interleaved (leg after leg inside every repetition), each window a pair of HIP events around `inner` back-to-back
calls; reported: median / min / max ms per call over the repetitions.  The interaction alone is timed the same way: the fused
launch (functional.gather_interact) against the pair it replaces (emb_offset_indices + emb_gather_fwd from the fp32 table +
dot_interact_fwd), with the achieved GB/s over the bytes each needs, computed here from the shapes.
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
from deeplearningexamples_amd.dlrm.infer import DlrmPredictor                          # noqa: E402
from deeplearningexamples_amd.dlrm.main import CRITEO_F15                              # noqa: E402
from deeplearningexamples_amd.dlrm.model import DistributedDlrm                        # noqa: E402

BATCHES = (1, 64, 4096, 65536)


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def interleaved(legs, inner, reps):
    """legs: name -> callable.  Every repetition runs every leg once, in turn -> name -> dict(median, min, max) in ms per call."""
    for fn in legs.values():                                  # warm every leg (code objects, graph capture, allocator)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(window(fn, inner))
    return {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}


def interaction_bytes(t, d, ow):
    """bytes per sample, from the shapes: the fused launch reads 1 + T 16-bit rows and T ids and writes the output row; the pair
    reads T fp32 rows, writes them as 16 bits, reads 1 + T 16-bit rows back and writes the output row (ids: read, rewritten as
    joint rows, read again)."""
    fused = (t + 1) * d * 2 + t * 8 + ow * 2
    pair = t * d * 4 + t * d * 2 + (t + 1) * d * 2 + ow * 2 + 3 * t * 8
    return fused, pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlrm_infer_perf.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    sizes = [min(s, a.cap) for s in CRITEO_F15]
    dim, dtype = 128, torch.float16
    model = DistributedDlrm(num_numerical_features=13, categorical_feature_sizes=sizes, bottom_mlp_sizes=[512, 256, 128],
                            top_mlp_sizes=[1024, 1024, 512, 256, 1], embedding_dim=dim, device=dev, compute_dtype=dtype)
    preds = {(fz, gr): DlrmPredictor(model, fused=fz, graphs=gr) for fz in (True, False) for gr in (False, True)}
    emb = model.bottom_model.embeddings
    table16 = preds[(True, False)].table16
    t = len(sizes)
    ow = F.dot_interact_out_width(t + 1, dim)
    per_fused, per_pair = interaction_bytes(t, dim, ow)
    g = torch.Generator().manual_seed(1)
    rows = []
    for b in BATCHES:
        num = torch.rand((b, 13), generator=g).to(dev)
        cat = torch.cat([torch.randint(0, s, (b, 1), generator=g) for s in sizes], 1).to(dev)
        inner = 200 if b <= 64 else (50 if b <= 4096 else 10)
        ref = preds[(True, False)].predict(num, cat).clone()
        for p in preds.values():
            assert torch.equal(p.predict(num, cat), ref), "the legs disagree"
        legs = {"%s_%s" % ("fused" if fz else "unfused", "graph" if gr else "eager"): (lambda p=p: p.predict(num, cat))
                for (fz, gr), p in preds.items()}
        res = interleaved(legs, inner, a.reps)
        # the interaction alone
        mlp = torch.randn((b, dim), generator=g).to(dtype).to(dev)
        x = torch.empty((b, t + 1, dim), dtype=dtype, device=dev)
        x[:, 0, :] = mlp
        out = torch.empty((b, ow), dtype=dtype, device=dev)

        def pair():
            r = F.emb_offset_indices(cat, emb.offsets, None)
            F.emb_gather_fwd(emb.weight.data, r, out_dtype=dtype, out=x[:, 1:, :], out_batch_stride=(t + 1) * dim)
            return F.dot_interact_fwd(x)

        def fused():
            return F.gather_interact(table16, cat, emb.offsets, None, mlp, out=out)
        assert torch.equal(fused(), pair()), "fused and unfused interaction disagree"
        ki = interleaved({"fused": fused, "pair": pair}, inner, a.reps)
        for k, per in (("fused", per_fused), ("pair", per_pair)):
            ki[k]["bytes_per_sample"] = per
            ki[k]["gb_per_s_at_median"] = per * b / (ki[k]["ms_median"] * 1e-3) / 1e9
        rows.append(dict(batch=b, inner=inner, reps=a.reps, predict=res, interaction=ki))
        print(json.dumps(rows[-1]), flush=True)
    result = dict(tool="tools/dlrm_infer_perf.py", device=torch.cuda.get_device_name(0), dtype="fp16", table_cap=a.cap,
                  joint_rows=int(sum(sizes)), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
