"""Worker of tests/test_gpu_dlrm_adam.py::test_two_ranks_adam_match_one_rank (NOT a test module): one rank of a 2-process
table-wise DLRM run with --Adam_embedding_optimizer and --Adam_MLP_optimizer.

    python -m torch.distributed.run --nproc-per-node 2 ... tests/_dlrm_adam_worker.py dlrm_adam <backend> <out.json>

The launcher, the process-group setup and the placement are those of tests/_multirank_worker.py (gloo staged through host
memory when both ranks share one GPU); only the optimizers differ.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _multirank_worker as W  # noqa: E402

ADAM_LR = 1e-3
# an eps near the size of the embedding gradients: Adam's update then depends on the gradient's scale, so a wrong 1 / world
# divisor changes the trajectory (with eps << |g| Adam is blind to it)
ADAM_EPS = 1e-4


def run_dlrm_adam(rank, world, dev, steps):
    """world 2: tables placed by get_device_mapping.  world 1: ONE rank holding the tables in the 2-rank DEVICE order, same
    weights, same batch (as _multirank_worker.run_dlrm), both optimizers Adam."""
    from oracle import dlrm_step_oracle as SO
    from deeplearningexamples_amd.dlrm import placement as P
    from deeplearningexamples_amd.dlrm.model import DistributedDlrm
    from deeplearningexamples_amd.dlrm.engine import DlrmTrainer
    c = W.DLRM_MR
    mapping2, order = W.dlrm_device_order(2)
    sizes_dev = [c["sizes"][t] for t in order]
    state = SO.seeded_dlrm_state(sizes_dev, c["dim"], c["bottom"], c["top"], c["num"], c["seed"])
    num, cat, click = SO.seeded_dlrm_batch(sizes_dev, c["num"], c["batch"], c["seed"] + 1)
    off = np.concatenate([[0], np.cumsum(sizes_dev)])
    if world == 1:
        my = list(range(len(sizes_dev)))
        has_bottom, vectors, batches = True, None, [c["batch"]]
    else:
        start = sum(len(b) for b in mapping2["embedding"][:rank])
        my = list(range(start, start + len(mapping2["embedding"][rank])))
        has_bottom = rank == mapping2["bottom_mlp"]
        vectors = mapping2["vectors_per_gpu"]
        batches = P.get_gpu_batch_sizes(c["batch"], world)
    torch.manual_seed(300 + rank)
    model = DistributedDlrm(num_numerical_features=c["num"], categorical_feature_sizes=[sizes_dev[i] for i in my],
                            bottom_mlp_sizes=c["bottom"] if has_bottom else None, top_mlp_sizes=c["top"],
                            vectors_per_gpu=vectors, embedding_device_mapping=mapping2["embedding"] if world > 1 else None,
                            world_num_categorical_features=len(sizes_dev), embedding_dim=c["dim"], device=dev,
                            compute_dtype=torch.float16, world_size=world)
    with torch.no_grad():
        if has_bottom:
            for i, l in enumerate(model.bottom_model.mlp.linears):
                l.weight.copy_(state["bottom_mlp.%d.weight" % i]); l.bias.copy_(state["bottom_mlp.%d.bias" % i])
        if rank == 0:
            for i, l in enumerate(model.top_model.mlp.linears):
                l.weight.copy_(state["top_mlp.%d.weight" % i]); l.bias.copy_(state["top_mlp.%d.bias" % i])
            model.top_model.out.weight.copy_(state["out.weight"]); model.top_model.out.bias.copy_(state["out.bias"])
        if my:
            rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in my])
            model.bottom_model.embeddings.weight.copy_(state["embedding"][torch.from_numpy(rows)])
    model.refresh_working_copies()
    probe_ids = {}
    if my:
        loc = np.concatenate([[0], np.cumsum([sizes_dev[i] for i in my])])
        for j, t in enumerate(my):
            probe_ids[str(t)] = torch.from_numpy(np.unique(cat[:, t].numpy())[:4] + loc[j]).to(dev)
    emb_init = {t: model.bottom_model.embeddings.weight.detach()[ids].clone() for t, ids in probe_ids.items()}
    tr = DlrmTrainer(model, lr=ADAM_LR, batch_sizes_per_gpu=batches, vectors_per_gpu=vectors, rank=rank, world_size=world,
                     amp=True, adam_embeddings=True, adam_mlps=True, adam_eps=ADAM_EPS)
    numd = num.to(dev) if has_bottom else None
    catd = cat[:, my].contiguous().to(dev) if my else None
    clickd = click.to(dev)
    losses = []
    for _ in range(steps):
        loss = tr.train_step(numd, catd, clickd)
        if world > 1:
            from deeplearningexamples_amd.utils import comm
            loss = comm.allreduce_mean_(loss.clone())
        losses.append(float(loss.item()))
    probe = model.top_model.out.weight.detach().float().cpu().numpy().reshape(-1)[:8].tolist()
    # movement (final - initial) of looked-up embedding rows by DEVICE-ORDER table index (each table lives on one rank)
    emb_rows = {}
    for t, ids in probe_ids.items():
        d = model.bottom_model.embeddings.weight.detach()[ids] - emb_init[t]
        emb_rows[t] = d.float().cpu().numpy()[:, :16].tolist()
    rates = {"lr_emb": float(tr.lr_emb.item()) if my else None, "emb_div": getattr(tr, "emb_div", None),
             "lr_mlp": float(tr.lr_mlp.item()), "mlp_gmul": tr.mlp_gmul.cpu().tolist(),
             "n_top_tensors": 2 * len(tr.top_linears), "has_bottom": has_bottom}
    return {"losses": losses, "probe": probe, "emb_rows": emb_rows, "rates": rates,
            "steps": [int(tr.emb_step.item()), int(tr.mlp_step.item())]}


W.SCENARIOS["dlrm_adam"] = run_dlrm_adam

if __name__ == "__main__":
    W.main()
