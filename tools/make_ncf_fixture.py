"""Writes the NCF fixtures under tests/golden/ from a checkout of the reference recipe (CPU only).  Recorded data only: results of
the reference's programs, never their text.

    python tools/make_ncf_fixture.py --reference /path/to/DeepLearningExamples/PyTorch/Recommendation/NCF

  ncf_state_dict.json   parameter names and shapes of the reference's NeuMF at the ml-20m sizes and at the fixture's
  ncf_cli_flags.json    flags, defaults and kinds of the reference's inference.py and ncf.py parsers
  ncf_eval.npz          a small model's test set (61 users, 211 items, 96 series of 100, one positive each, items duplicated
                        inside a series -- the positive too, in every fourth series), the reference NeuMF's float64 logits on it,
                        what the reference's TestDataLoader makes of it (sorted users / items / labels, duplicate mask) and
                        val_epoch's hr, ndcg and loss in float64
  ncf_checkpoint.pt     that model's state dict under DistributedDataParallel's `module.` prefix

The model is tests/_ncf_ref.seeded_state(61, 211, SEED): tables N(0, 1), biases U(-0.1, 0.1), so the logits spread over several
units (with the reference's 0.01 tables every logit is about -0.11 and nothing can be ranked).  The reference's dataset class loads
to cuda:0: the loader is fed a stub dataset on the CPU.  dllogger and apex are stubbed in sys.modules.
"""
import argparse
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_USERS, N_ITEMS, N_SERIES, S, K, SEED, VALID_BATCH = 61, 211, 96, 100, 10, 2024, 2048


def reference_modules(ref):
    for name in ("dllogger", "apex", "apex.optimizers"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["apex.optimizers"].FusedAdam = object
    sys.modules["apex"].optimizers = sys.modules["apex.optimizers"]
    sys.path.insert(0, ref)
    import dataloading
    import feature_spec
    import ncf
    import neumf
    return neumf, dataloading, feature_spec, ncf


def parser_flags(path):
    """(flags, default, action, type, nargs, choices) of every add_argument call of a reference command line, from its syntax tree."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            lit = lambda k: eval(compile(ast.Expression(kw[k]), path, "eval"), {"__builtins__": {}}) if k in kw else None
            action = lit("action")
            out.append({"flags": [ast.literal_eval(a) for a in node.args], "default": False if action == "store_true" and "default" not in kw
                        else lit("default"), "action": action, "type": getattr(kw.get("type"), "id", None), "nargs": lit("nargs"),
                        "choices": lit("choices")})
    return out


def test_set(torch):
    g = torch.Generator().manual_seed(SEED + 1)
    users = (torch.arange(N_SERIES) % N_USERS).view(-1, 1).expand(N_SERIES, S).contiguous()
    items = torch.randint(0, N_ITEMS, (N_SERIES, S), generator=g)                  # 99 draws of 211 with replacement: duplicates
    for s in range(N_SERIES):
        while int((items[s, 1:] == items[s, 0]).sum()):                            # the positive is no accidental duplicate ...
            items[s, 1:] = torch.where(items[s, 1:] == items[s, 0], torch.randint(0, N_ITEMS, (S - 1,), generator=g), items[s, 1:])
        if s % 4 == 0:
            items[s, 37] = items[s, 0]                                              # ... but a deliberate one in every fourth series
    labels = torch.zeros(N_SERIES, S)
    labels[:, 0] = 1.0                                                              # positives first, as the reference's converter writes
    return users.reshape(-1, 1), items.reshape(-1, 1), labels.reshape(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    neumf, dataloading, feature_spec, ncf = reference_modules(args.reference)
    import torch
    from tests import _ncf_ref as R
    from tests import _tft_ref as T
    os.makedirs(GOLDEN, exist_ok=True)

    # 1. names and shapes
    shapes = {}
    for tag, (nu, ni) in (("ml-20m", (138493, 26744)), ("fixture", (N_USERS, N_ITEMS))):
        m = neumf.NeuMF(nu, ni, 64, [256, 256, 128, 64], 0.5)
        shapes[tag] = {k: list(v.shape) for k, v in m.state_dict().items()}
    json.dump(shapes, open(os.path.join(GOLDEN, "ncf_state_dict.json"), "w"), indent=1)

    # 2. the two command lines
    json.dump({"inference": parser_flags(os.path.join(args.reference, "inference.py")),
               "ncf": parser_flags(os.path.join(args.reference, "ncf.py"))}, open(os.path.join(GOLDEN, "ncf_cli_flags.json"), "w"), indent=1)

    # 3. the small model, its float64 forward, the loader and val_epoch
    sd = R.seeded_state(N_USERS, N_ITEMS, SEED)
    model = neumf.NeuMF(N_USERS, N_ITEMS, 64, [256, 256, 128, 64], 0.0)
    model.load_state_dict(sd)
    model = model.double().eval()
    users, items, labels = test_set(torch)
    with torch.no_grad():
        logit64 = model(users.view(-1), items.view(-1)).view(-1)
    spec = feature_spec.FeatureSpec.from_dict(
        {"feature_spec": {"user": {"dtype": "torch.int64", "cardinality": N_USERS}, "item": {"dtype": "torch.int64", "cardinality": N_ITEMS},
                          "label": {"dtype": "torch.float32"}},
         "source_spec": {"test": []}, "channel_spec": {"user_ch": ["user"], "item_ch": ["item"], "label_ch": ["label"]},
         "metadata": {"test_samples_per_series": S}}, base_directory="")
    stub = types.SimpleNamespace(feature_spec=spec, features={"user": users.clone(), "item": items.clone(), "label": labels.double()})
    largs = types.SimpleNamespace(world_size=1, local_rank=0, valid_batch_size=VALID_BATCH)
    loader = dataloading.TestDataLoader(stub, largs)
    # val_epoch takes the logarithm of the ranks after `.to(torch.float)`: for the duration of the call that name is float64, so the
    # recorded ndcg is the float64 value of its formula, not an fp32 rounding of it
    f32, torch.float = torch.float, torch.float64
    try:
        hr, ndcg, loss = ncf.val_epoch(model, loader, K)
    finally:
        torch.float = f32
    s_users, s_items, s_labels = (loader.data[c][n].view(-1) for c, n in (("user_ch", "user"), ("item_ch", "item"), ("label_ch", "label")))
    mask = loader.get_ignore_mask().view(-1)
    with torch.no_grad():
        s_logit64 = model(s_users, s_items).view(-1)

    # its own assertions: no rating ties with a label-1 element; at least 90 % of the series boundary-clear in both 16-bit types
    r = torch.sigmoid(s_logit64).view(-1, S).clone()
    r[mask.view(-1, S)] = -1
    lab = s_labels.view(-1, S) == 1
    for s in range(N_SERIES):
        for j in torch.nonzero(lab[s]).flatten().tolist():
            assert int((r[s] == r[s, j]).sum()) == 1, "series %d: a rating ties with the positive's" % s
    clear = {}
    for dtype in (torch.float16, torch.bfloat16):
        e_emul = float((R.half_forward(sd, s_users, s_items, dtype) - s_logit64).abs().max())
        c = R.boundary_clear(s_logit64, s_labels, mask, S, K, 8 * e_emul)
        clear[str(dtype)] = (e_emul, float(c.double().mean()))
        assert c.double().mean() >= 0.9, (dtype, e_emul, float(c.double().mean()))
    print("E_emulated and the clear fraction:", clear, " hr %.6f ndcg %.6f loss %.6f" % (hr, ndcg, float(loss)))
    np.savez_compressed(os.path.join(GOLDEN, "ncf_eval.npz"), seed=SEED, n_users=N_USERS, n_items=N_ITEMS, samples_in_series=S, k=K,
                        valid_batch_size=VALID_BATCH, users=users.view(-1).numpy(), items=items.view(-1).numpy(),
                        labels=labels.view(-1).numpy().astype(np.float32), logit64=logit64.numpy(),
                        sorted_users=s_users.numpy(), sorted_items=s_items.numpy(), sorted_labels=s_labels.numpy().astype(np.float32),
                        mask=mask.numpy(), sorted_logit64=s_logit64.numpy(), hr=np.float64(hr), ndcg=np.float64(ndcg),
                        loss=np.float64(float(loss)), n_batches=len(loader.get_epoch_data()))

    # 4. the checkpoint, as DistributedDataParallel saves it
    torch.save({"module." + k: v.clone() for k, v in sd.items()}, os.path.join(GOLDEN, "ncf_checkpoint.pt"))
    for f in ("ncf_state_dict.json", "ncf_cli_flags.json", "ncf_eval.npz", "ncf_checkpoint.pt"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
