"""DLRM step time with SGD vs Adam at the bench's DLRM configuration (criteo_f15, 26 tables x dim 128, fp16 AMP, batch 65536,
one GPU): SGD, embedding Adam, MLP Adam and both, timed with device events in alternating rounds in ONE process over one
model (each optimizer set is its own DlrmTrainer).  Prints one JSON line: ms / step per variant, the distinct rows the batch
touches and the algorithmic bytes of the sparse updates (Adam: touched rows x 6 x dim x 4 + lookups x (dim x 2 + 8); SGD:
lookups x (dim x 2 + 8) + touched rows x 2 x dim x 4).

    python tools/dlrm_adam_step.py [--steps 20] [--warmup 5] [--rounds 3] [--only sgd,emb,mlp,both]

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/dlrm_adam_step.py --only both` and read the
emb_adam_* / emb_onehot_kernel / mt_adam_copy rows of the stats table.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CRITEO_F15 = [7912889, 33823, 582469, 245828, 11, 2209, 10667, 104, 4, 968, 15, 8165896, 17139,
              2675940, 7156453, 302516, 12022, 97, 35, 7339, 20046, 4, 7105, 1382, 63, 5554114]
VARIANTS = {"sgd": (False, False), "emb": (True, False), "mlp": (False, True), "both": (True, True)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--only", default="sgd,emb,mlp,both")
    a = ap.parse_args(argv)
    from deeplearningexamples_amd.dlrm.model import DistributedDlrm
    from deeplearningexamples_amd.dlrm.engine import DlrmTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(12345)
    model = DistributedDlrm(num_numerical_features=13, categorical_feature_sizes=CRITEO_F15, bottom_mlp_sizes=[512, 256, 128],
                            top_mlp_sizes=[1024, 1024, 512, 256, 1], embedding_dim=128, device=dev, compute_dtype=torch.float16)
    g = torch.Generator(device="cpu").manual_seed(2024)                # the bench's synthetic batch
    num = torch.rand((a.batch, 13), generator=g).to(dev)
    cat = torch.cat([torch.randint(0, s, (a.batch, 1), generator=g) for s in CRITEO_F15], dim=1).to(dev)
    click = torch.randint(0, 2, (a.batch,), generator=g).float().to(dev)
    names = [n for n in a.only.split(",") if n]
    # (small rates: the timed steps must not overflow, a skipped step would time less work)
    trainers = {n: DlrmTrainer(model, lr=1e-3 if n != "sgd" else 1e-2, batch_sizes_per_gpu=[a.batch], amp=True,
                               adam_embeddings=VARIANTS[n][0], adam_mlps=VARIANTS[n][1]) for n in names}
    for n in names:
        for _ in range(a.warmup):
            trainers[n].train_step(num, cat, click)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    skipped = {n: 0 for n in names}
    for _ in range(a.rounds):
        for n in names:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                trainers[n].train_step(num, cat, click)
            e.record()
            torch.cuda.synchronize()
            ms[n].append(s.elapsed_time(e) / a.steps)
            skipped[n] += int(trainers[n].scaler.scale.item() < 65536.0)
    off = model.bottom_model.embeddings.offsets[:-1]
    touched = int(torch.unique((cat + off).reshape(-1)).numel())
    lookups = a.batch * len(CRITEO_F15)
    d = 128
    out = {"ms_per_step": {n: min(v) for n, v in ms.items()}, "ms_rounds": ms, "scale_backed_off": skipped,
           "touched_rows": touched, "lookups": lookups,
           "adam_sparse_bytes": touched * 6 * d * 4 + lookups * (d * 2 + 8),
           "sgd_sparse_bytes": touched * 2 * d * 4 + lookups * (d * 2 + 8),
           "adam_state_bytes": 2 * int(model.bottom_model.embeddings.weight.numel()) * 4}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
