"""NCF inference timing: NeuMF at the ml-20m sizes (138493 users, 26744 items, --factors 64 --layers 256 256 128 64), every batch
size of the reference's inference.py list, fp16 and bf16.

    python tools/ncf_infer_perf.py [--reps 7] [--out profiles/ncf_infer_perf.json]

Per dtype and batch size the four legs of NeuMFScorer.predict -- fused launch / unfused chain x eager launches / graph replay -- are
timed in ONE process, interleaved (leg after leg inside every repetition), each window a pair of HIP events around `inner`
back-to-back calls after three warm-up calls per leg; reported: median / min / max ms per call over the repetitions, and the
spread (max - min) / median.  The four F.rows_gather launches of the same samples on the same tables are timed the same way: the
run's own gather rate (768 table bytes per sample over their time).  The byte bound of a batch is 768 B per sample at the best
gather rate the run measured at any batch size; the fused launch's distance from it is reported, not gated.

Routing: a batch size stays on the fused route only if fused_eager is faster than unfused_eager by more than the larger spread
of the two legs, in both dtypes; the others are printed as the UNFUSED_BATCH_SIZES the run supports.
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
from deeplearningexamples_amd.ncf import infer as NI                                   # noqa: E402
from deeplearningexamples_amd.ncf.infer import NeuMFScorer                             # noqa: E402
from deeplearningexamples_amd.ncf.model import NeuMFModel                              # noqa: E402

BATCHES = (1, 4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576)
N_USERS, N_ITEMS = 138493, 26744
ROW_BYTES = 2 * (64 + 64 + 128 + 128)


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def interleaved(legs, inner, reps):
    """legs: name -> callable.  Every repetition runs every leg once, in turn -> name -> median / min / max ms per call, spread."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncf_infer_perf.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    NI.UNFUSED_BATCH_SIZES = frozenset()               # measure the fused launch at every size, whatever the current routing says
    model = NeuMFModel(N_USERS, N_ITEMS).eval()
    with torch.no_grad():                              # trained-size activations: the reference's 0.01 tables would leave the ReLUs to the biases
        for emb in (model.mf_user_embed, model.mf_item_embed, model.mlp_user_embed, model.mlp_item_embed):
            emb.weight.normal_(0.0, 1.0)
    g = torch.Generator().manual_seed(1)
    rows, losers = [], set()
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        sc = {(fz, gr): NeuMFScorer(model, dtype=dtype, fused=fz, graphs=gr) for fz in (True, False) for gr in (False, True)}
        tables = sc[(True, False)].tables
        for b in BATCHES:
            users = torch.randint(0, N_USERS, (b,), generator=g).to(dev)
            items = torch.randint(0, N_ITEMS, (b,), generator=g).to(dev)
            inner = 200 if b <= 1024 else (50 if b <= 65536 else 10)
            assert torch.equal(sc[(True, True)].predict(users, items), sc[(True, False)].predict(users, items))
            legs = {"%s_%s" % ("fused" if fz else "unfused", "graph" if gr else "eager"): (lambda p=p: p.predict(users, items))
                    for (fz, gr), p in sc.items()}
            res = interleaved(legs, inner, a.reps)
            gather = interleaved({"rows_gather_x4": lambda: [F.rows_gather(t, users if j % 2 == 0 else items) for j, t in enumerate(tables)]},
                                 inner, a.reps)["rows_gather_x4"]
            gather["gb_per_s_at_median"] = ROW_BYTES * b / (gather["ms_median"] * 1e-3) / 1e9
            fe, ue = res["fused_eager"], res["unfused_eager"]
            margin = max(fe["spread"], ue["spread"])
            keeps = fe["ms_median"] * (1.0 + margin) < ue["ms_median"]
            if not keeps:
                losers.add(b)
            rows.append(dict(dtype=name, batch=b, inner=inner, reps=a.reps, predict=res, gather=gather, margin=margin, fused_keeps_the_route=keeps,
                             samples_per_s_fused_eager=b / (fe["ms_median"] * 1e-3)))
            print(json.dumps(rows[-1]), flush=True)
    peak = max(r["gather"]["gb_per_s_at_median"] for r in rows)
    for r in rows:
        r["byte_bound_ms"] = ROW_BYTES * r["batch"] / (peak * 1e9) * 1e3
        r["fused_eager_over_byte_bound"] = r["predict"]["fused_eager"]["ms_median"] / r["byte_bound_ms"]
    result = dict(tool="tools/ncf_infer_perf.py", device=torch.cuda.get_device_name(0), n_users=N_USERS, n_items=N_ITEMS,
                  table_bytes_16bit=(N_USERS + N_ITEMS) * (64 + 128) * 2, row_bytes_per_sample=ROW_BYTES, peak_gather_gb_per_s=peak,
                  unfused_batch_sizes=sorted(losers), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("UNFUSED_BATCH_SIZES supported by this run:", sorted(losers))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
